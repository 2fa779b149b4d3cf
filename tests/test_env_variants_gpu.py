"""The kernel variants that still sit behind environment switches (read once per process by the library)
run the convolution parity tests in child processes, so that a non-default path cannot rot unnoticed:
  S2S_CONV_XCD=0, S2S_WGRAD_XCD=0   plain (not XCD-aware) workgroup order
  S2S_WGRAD_BLOCKS=512    two weight-gradient workgroups per CU (default: one), without the fill rule
  S2S_CONV_PERS=0         one tile per workgroup also for the >= 1024-tile launches (default: persistent tile walk)
  S2S_CONV_STAGE=0 / 2    no launch / every eligible launch on the staged kernel (default 1: filter-resident and
                          single-channel-tile launches)
(Round 4 deleted what rounds 2-3 had measured and dropped: S2S_WGRAD_KH, S2S_WGRAD_MFMA, S2S_WGRAD_DMA, S2S_CONV_EPI and
the tuning knobs whose sweeps ended at their defaults; S2S_CONV_DMA and S2S_CONV_CFG followed.)
A child takes 46 to 50 s on an MI355X (tests/test_conv3x3_forms_gpu.py is 20 to 25 s of it), well inside its 900 s."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = [{"S2S_CONV_XCD": "0", "S2S_WGRAD_XCD": "0"}, {"S2S_WGRAD_BLOCKS": "512"}, {"S2S_CONV_PERS": "0"}, {"S2S_CONV_STAGE": "0"}, {"S2S_CONV_STAGE": "2"}]
# (The result-changing S2S_CONV_DBG timing bits are NOT in the product library: they are compiled only with -DS2S_ABLATE
#  into libstain2stain_hip_ablate.so, which scripts/ load; tests/test_native_cpu.py checks that the shipped sources read no
#  such switch outside that guard.)


@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join(f"{k[4:]}={v}" for k, v in e.items()))
def test_conv_parity_under_switch(env):
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                          os.path.join(ROOT, "tests", "test_ops_gpu.py"), os.path.join(ROOT, "tests", "test_fuzz_gpu.py"),
                          os.path.join(ROOT, "tests", "test_unwritten_memory_gpu.py"),
                          os.path.join(ROOT, "tests", "test_wgrad_forms_gpu.py"),
                          os.path.join(ROOT, "tests", "test_conv3x3_forms_gpu.py"),
                          "-k", "conv3x3 or random_shapes"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env={**os.environ, **env})
    assert out.returncode == 0, out.stdout[-2500:] + out.stderr[-1500:]
    assert " passed" in out.stdout and "failed" not in out.stdout
