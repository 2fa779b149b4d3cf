"""CPU-side checks of the native boundary: the library builds for gfx950, loads, and exports exactly the
symbols include/stain2stain_hip.h declares; host-side argument validation returns negative status codes
without touching a GPU; the drop-in modules keep the reference's state_dict contract."""
import ctypes
import os

import pytest
import torch

from conftest import load_golden, sub


def test_library_builds_loads_and_exports_every_declared_symbol():
    from stain2stain_amd import _native
    _native.build()
    assert os.path.exists(_native.LIB_PATH)
    lib = _native.lib()
    names = _native.declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), n


def test_host_side_validation_returns_status_codes_without_a_gpu():
    from stain2stain_amd import _native
    lib = _native.lib()
    # null pointers / bad shapes are rejected before any launch
    assert lib.s2s_conv3x3_nhwc(0, None, 8, 8, None, 8, 0, None, None, None, 8, None, None, None, 0, 1, 4, 4, 8, None) == -5
    # output side of the conv ABI: Cout / ldy multiples of 8, ldy >= Cout, 16-byte aligned y -- the
    # epilogue stores whole 16-byte pieces, so anything else must be refused, not written out of bounds
    ok = ctypes.c_void_p(4096)
    conv = lambda cout, ldy, y: lib.s2s_conv3x3_nhwc(0, ok, 8, 8, None, 8, 0, ok, None, y, ldy, None, None, None, 0,
                                                      1, 4, 4, cout, None)
    assert conv(12, 16, ok) == -1 and conv(8, 12, ok) == -1 and conv(16, 8, ok) == -1
    assert conv(8, 8, ctypes.c_void_p(4096 + 8)) == -2
    assert lib.s2s_conv3x3_stat_blocks(0, 16, 256, 256, 64) == 16 * 32 * 8 * 4      # (tile, wave row) rows: 8x32x64 tile, 4 x 1 waves
    assert lib.s2s_conv3x3_stat_blocks(1, 16, 256, 256, 64) == 16 * 64 * 8
    assert lib.s2s_conv3x3_stat_blocks(7, 1, 8, 8, 8) == -3
    assert lib.s2s_conv3x3_wgrad_splits(0, 16, 256, 256, 64, 64) >= 1
    assert lib.s2s_conv3x3_wgrad_splits(0, 0, 1, 1, 8, 8) == -1
    assert lib.s2s_pack_conv3x3_fwd_elems(64, 48) == 9 * 2 * 64 * 32
    assert lib.s2s_pack_conv3x3_dgrad_elems(64, 48) == 9 * 2 * 48 * 32
    assert lib.s2s_bn_bwd_blocks(2, 0, 4, 8) == -1
    assert lib.s2s_adam_step(None, None, None, None, 10, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None) == -5


def test_error_status_becomes_runtime_error():
    from stain2stain_amd import _native
    with pytest.raises(RuntimeError, match="null pointer"):
        _native.check(-5, "op")
    _native.check(0, "op")


def test_modules_keep_reference_state_dict_and_init(golden_tiny, golden_odd3):
    from stain2stain_amd import FlowUNet
    for G, feats, tdim in ((golden_tiny, [16, 32], 32), (golden_odd3, [8, 16, 24], 16)):
        torch.manual_seed(1984)
        net = FlowUNet(3, feats, 3, tdim)
        ref = sub(G, "init/")
        sd = net.state_dict()
        assert set(sd) == set(ref)
        for k, v in ref.items():
            assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, k
            assert torch.equal(sd[k], v), k         # same construction order => same RNG consumption
        net.load_state_dict(sub(G, "step0/after/"), strict=True)


def test_no_cpu_fallback():
    from stain2stain_amd import FlowUNet, SharedEncoder
    with pytest.raises(RuntimeError):
        FlowUNet(3, [16, 32], 3, 32)(torch.rand(2), torch.rand(2, 3, 16, 16))
    with pytest.raises(ValueError):
        SharedEncoder(3, [12, 20])           # channel widths must be multiples of 8
    with pytest.raises(ValueError):
        SharedEncoder(3, [16, 32], precision="fp16")


def test_product_path_never_imports_the_oracle():
    """The oracle is test infrastructure: no module of the shipped package may import it."""
    import re
    import stain2stain_amd
    root = stain2stain_amd.__path__[0]
    for fn in os.listdir(root):
        if fn.endswith(".py"):
            src = open(os.path.join(root, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), fn


def test_unloadable_library_fails_loudly(tmp_path, monkeypatch):
    """No silent fallback when the HIP library cannot be loaded: the first op raises and names the file."""
    from stain2stain_amd import _native
    bad = tmp_path / "libstain2stain_hip.so"
    bad.write_bytes(b"not an ELF file")
    monkeypatch.setattr(_native, "LIB_PATH", str(bad))
    monkeypatch.setattr(_native, "_lib", None)
    with pytest.raises(RuntimeError, match="cannot load"):
        _native.lib()


def test_product_library_reads_only_result_preserving_switches():
    """the timing ablations that produce wrong results (S2S_CONV_DBG bits 1-32) must not be reachable
    in the shipped library through an environment variable, and the superseded forward loops (S2S_CONV_DMA) are gone.
    Preprocess every source WITHOUT -DS2S_ABLATE (comments stripped, #ifdef S2S_ABLATE blocks dropped) and look at what
    is left: no S2S_CONV_DMA read at all, and the S2S_CONV_DBG read masked to the clock probe (64), the one debug bit
    the shipped library still has."""
    import re
    from stain2stain_amd import _native

    def product_text(path):
        out, skip = [], 0
        for line in open(path).read().splitlines():
            st = line.strip()
            if skip:
                if st.startswith("#if"):
                    skip += 1
                elif st.startswith("#else") and skip == 1:
                    skip = 0
                elif st.startswith("#endif"):
                    skip -= 1
                continue
            if st.startswith("#ifdef S2S_ABLATE"):
                skip = 1
                continue
            out.append(re.sub(r"//.*", "", line))
        return "\n".join(out)

    envs = {}
    for src in _native.SOURCES:
        text = product_text(os.path.join(_native.CSRC, src))
        for name in re.findall(r'getenv\("(S2S_\w+)"\)', text):
            envs.setdefault(name, []).append(src)
        if "S2S_CONV_DBG" in text:
            assert re.search(r'getenv\("S2S_CONV_DBG"\).*& S2S_DBG_MASK', text), src
            assert re.search(r"#define S2S_DBG_MASK \(?64\)?\s*$", text, re.M), src
        assert not re.search(r"a\.dbg & (1|2|4|8|16|32)\b(?!\d)", re.sub(r"S2S_ABL\([^)]*\)", "", text)), src
    assert "S2S_CONV_DMA" not in envs, envs.get("S2S_CONV_DMA")
    # what remains is result-preserving (tile choice, workgroup order, split counts, equivalent kernels): each is either
    # exercised by tests/test_env_variants_gpu.py or changes launch geometry only
    allowed = {"S2S_CONV_DBG", "S2S_CONV_PERS", "S2S_CONV_STAGE", "S2S_CONV_XCD", "S2S_WGRAD_XCD", "S2S_WGRAD_BLOCKS",
               "S2S_P2P_WGRAD_BLOCKS", "S2S_P2P_WGRAD_S1_BLOCKS", "S2S_UP_BAND"}
    assert len(allowed) <= 12          # what was measured and dropped is deleted, not switched off
    assert set(envs) <= allowed, set(envs) - allowed


# The launch-plan queries of the 3x3 convolution (s2s_conv3x3_stat_blocks / _ksplit / _stat_rows / _staged), pinned to
# the values of the library before the plan was gathered into one function.  Columns: dtype, B, H, W, Cout, c0, c1, ld0,
# ld1, has_bias | stat_blocks, ksplit(cin = c0 + c1) | (stat_rows, staged without / with statistics) with no switch set,
# with S2S_CONV_STAGE=0, S2S_CONV_STAGE=2 and S2S_CONV_PERS=0.  Rows: the CFM U-Net levels at batch 16 and 2 (encoder,
# a data gradient, the decoder's two-source conv from its concat buffer), the multitask 512^2 x 8 levels, two sources
# with c0 % 32 != 0, fp32, a bias.
CONV3X3_QUERY_ENVS = [{}, {"S2S_CONV_STAGE": "0"}, {"S2S_CONV_STAGE": "2"}, {"S2S_CONV_PERS": "0"}]
CONV3X3_QUERIES = [
    (0, 16, 256, 256, 64, 64, 0, 64, 0, 0, 16384, 1, (2048, 2, 2), (2048, 0, 0), (2048, 2, 2), (2048, 2, 2)),
    (0, 16, 256, 256, 64, 64, 64, 128, 128, 0, 16384, 1, (2048, 1, 1), (2048, 0, 0), (2048, 1, 1), (2048, 1, 1)),
    (0, 16, 128, 128, 128, 64, 0, 64, 0, 0, 2048, 1, (2048, 2, 2), (2048, 0, 0), (2048, 2, 2), (2048, 2, 2)),
    (0, 16, 128, 128, 128, 128, 0, 128, 0, 0, 2048, 1, (2048, 0, 0), (2048, 0, 0), (2048, 1, 1), (2048, 0, 0)),
    (0, 16, 128, 128, 64, 128, 0, 128, 0, 0, 4096, 1, (2048, 1, 1), (2048, 0, 0), (2048, 1, 1), (2048, 1, 1)),
    (0, 16, 128, 128, 128, 128, 128, 256, 256, 0, 2048, 1, (2048, 0, 0), (2048, 0, 0), (2048, 1, 1), (2048, 0, 0)),
    (0, 16, 64, 64, 256, 128, 0, 128, 0, 0, 512, 1, (512, 0, 0), (512, 0, 0), (2048, 1, 1), (512, 0, 0)),
    (0, 16, 64, 64, 256, 256, 0, 256, 0, 0, 512, 1, (512, 0, 0), (512, 0, 0), (2048, 1, 1), (512, 0, 0)),
    (0, 16, 64, 64, 128, 256, 0, 256, 0, 0, 1024, 1, (1024, 0, 0), (1024, 0, 0), (1024, 0, 0), (1024, 0, 0)),
    (0, 16, 64, 64, 256, 256, 256, 512, 512, 0, 512, 1, (512, 0, 0), (512, 0, 0), (2048, 1, 1), (512, 0, 0)),
    (0, 16, 32, 32, 512, 256, 0, 256, 0, 0, 256, 1, (256, 0, 0), (256, 0, 0), (256, 0, 0), (256, 0, 0)),
    (0, 16, 32, 32, 512, 512, 0, 512, 0, 0, 256, 1, (256, 0, 0), (256, 0, 0), (256, 0, 0), (256, 0, 0)),
    (0, 16, 32, 32, 256, 512, 0, 512, 0, 0, 256, 1, (256, 0, 0), (256, 0, 0), (256, 0, 0), (256, 0, 0)),
    (0, 16, 32, 32, 512, 512, 512, 1024, 1024, 0, 256, 1, (256, 0, 0), (256, 0, 0), (256, 0, 0), (256, 0, 0)),
    (0, 16, 16, 16, 1024, 512, 0, 512, 0, 0, 64, 1, (64, 0, 0), (64, 0, 0), (64, 0, 0), (64, 0, 0)),
    (0, 16, 16, 16, 1024, 1024, 0, 1024, 0, 0, 64, 1, (64, 0, 0), (64, 0, 0), (64, 0, 0), (64, 0, 0)),
    (0, 16, 16, 16, 512, 1024, 0, 1024, 0, 0, 64, 1, (64, 0, 0), (64, 0, 0), (64, 0, 0), (64, 0, 0)),
    (0, 16, 16, 16, 1024, 1024, 1024, 2048, 2048, 0, 64, 1, (64, 0, 0), (64, 0, 0), (64, 0, 0), (64, 0, 0)),
    (0, 16, 256, 256, 192, 64, 0, 64, 0, 0, 16384, 1, (2048, 2, 2), (16384, 0, 0), (2048, 2, 2), (2048, 2, 2)),
    (0, 16, 256, 256, 64, 192, 0, 192, 0, 0, 16384, 1, (2048, 1, 1), (2048, 0, 0), (2048, 1, 1), (2048, 1, 1)),
    (0, 2, 256, 256, 64, 64, 0, 64, 0, 0, 2048, 1, (2048, 0, 0), (2048, 0, 0), (2048, 0, 0), (2048, 0, 0)),
    (0, 2, 256, 256, 64, 64, 64, 128, 128, 0, 2048, 1, (2048, 0, 0), (2048, 0, 0), (2048, 0, 0), (2048, 0, 0)),
    (0, 2, 128, 128, 128, 64, 0, 64, 0, 0, 512, 1, (512, 0, 0), (512, 0, 0), (512, 0, 0), (512, 0, 0)),
    (0, 2, 128, 128, 128, 128, 0, 128, 0, 0, 512, 1, (512, 0, 0), (512, 0, 0), (512, 0, 0), (512, 0, 0)),
    (0, 2, 128, 128, 64, 128, 0, 128, 0, 0, 512, 1, (512, 0, 0), (512, 0, 0), (512, 0, 0), (512, 0, 0)),
    (0, 2, 128, 128, 128, 128, 128, 256, 256, 0, 512, 1, (512, 0, 0), (512, 0, 0), (512, 0, 0), (512, 0, 0)),
    (0, 2, 64, 64, 256, 128, 0, 128, 0, 0, 128, 1, (128, 0, 0), (128, 0, 0), (128, 0, 0), (128, 0, 0)),
    (0, 2, 64, 64, 256, 256, 0, 256, 0, 0, 128, 1, (128, 0, 0), (128, 0, 0), (128, 0, 0), (128, 0, 0)),
    (0, 2, 64, 64, 128, 256, 0, 256, 0, 0, 128, 1, (128, 0, 0), (128, 0, 0), (128, 0, 0), (128, 0, 0)),
    (0, 2, 64, 64, 256, 256, 256, 512, 512, 0, 128, 1, (128, 0, 0), (128, 0, 0), (128, 0, 0), (128, 0, 0)),
    (0, 2, 32, 32, 512, 256, 0, 256, 0, 0, 32, 1, (32, 0, 0), (32, 0, 0), (32, 0, 0), (32, 0, 0)),
    (0, 2, 32, 32, 512, 512, 0, 512, 0, 0, 32, 1, (32, 0, 0), (32, 0, 0), (32, 0, 0), (32, 0, 0)),
    (0, 2, 32, 32, 256, 512, 0, 512, 0, 0, 32, 4, (32, 0, 0), (32, 0, 0), (32, 0, 0), (32, 0, 0)),
    (0, 2, 32, 32, 512, 512, 512, 1024, 1024, 0, 32, 1, (32, 0, 0), (32, 0, 0), (32, 0, 0), (32, 0, 0)),
    (0, 2, 16, 16, 1024, 512, 0, 512, 0, 0, 8, 4, (8, 0, 0), (8, 0, 0), (8, 0, 0), (8, 0, 0)),
    (0, 2, 16, 16, 1024, 1024, 0, 1024, 0, 0, 8, 8, (8, 0, 0), (8, 0, 0), (8, 0, 0), (8, 0, 0)),
    (0, 2, 16, 16, 512, 1024, 0, 1024, 0, 0, 8, 8, (8, 0, 0), (8, 0, 0), (8, 0, 0), (8, 0, 0)),
    (0, 2, 16, 16, 1024, 1024, 1024, 2048, 2048, 0, 8, 8, (8, 0, 0), (8, 0, 0), (8, 0, 0), (8, 0, 0)),
    (0, 2, 256, 256, 192, 64, 0, 64, 0, 0, 2048, 1, (2048, 2, 2), (2048, 0, 0), (2048, 2, 2), (2048, 2, 2)),
    (0, 2, 256, 256, 64, 192, 0, 192, 0, 0, 2048, 1, (2048, 0, 0), (2048, 0, 0), (2048, 0, 0), (2048, 0, 0)),
    (0, 8, 512, 512, 64, 64, 0, 64, 0, 0, 32768, 1, (2048, 2, 2), (2048, 0, 0), (2048, 2, 2), (2048, 2, 2)),
    (0, 8, 512, 512, 64, 64, 64, 128, 128, 0, 32768, 1, (2048, 1, 1), (2048, 0, 0), (2048, 1, 1), (2048, 1, 1)),
    (0, 8, 256, 256, 128, 64, 0, 64, 0, 0, 4096, 1, (2048, 2, 2), (4096, 0, 0), (2048, 2, 2), (2048, 2, 2)),
    (0, 8, 256, 256, 128, 128, 0, 128, 0, 0, 4096, 1, (4096, 0, 0), (4096, 0, 0), (2048, 1, 1), (4096, 0, 0)),
    (0, 8, 256, 256, 128, 128, 128, 256, 256, 0, 4096, 1, (4096, 0, 0), (4096, 0, 0), (2048, 1, 1), (4096, 0, 0)),
    (0, 8, 128, 128, 256, 128, 0, 128, 0, 0, 1024, 1, (1024, 0, 0), (1024, 0, 0), (2048, 1, 1), (1024, 0, 0)),
    (0, 8, 128, 128, 256, 256, 0, 256, 0, 0, 1024, 1, (1024, 0, 0), (1024, 0, 0), (2048, 1, 1), (1024, 0, 0)),
    (0, 8, 128, 128, 256, 256, 256, 512, 512, 0, 1024, 1, (1024, 0, 0), (1024, 0, 0), (2048, 1, 1), (1024, 0, 0)),
    (0, 8, 64, 64, 512, 256, 0, 256, 0, 0, 256, 1, (256, 0, 0), (256, 0, 0), (2048, 1, 1), (256, 0, 0)),
    (0, 8, 64, 64, 512, 512, 0, 512, 0, 0, 256, 1, (256, 0, 0), (256, 0, 0), (2048, 1, 1), (256, 0, 0)),
    (0, 8, 64, 64, 512, 512, 512, 1024, 1024, 0, 256, 1, (256, 0, 0), (256, 0, 0), (2048, 1, 1), (256, 0, 0)),
    (0, 8, 32, 32, 1024, 512, 0, 512, 0, 0, 128, 1, (128, 0, 0), (128, 0, 0), (128, 0, 0), (128, 0, 0)),
    (0, 8, 32, 32, 1024, 1024, 0, 1024, 0, 0, 128, 1, (128, 0, 0), (128, 0, 0), (128, 0, 0), (128, 0, 0)),
    (0, 8, 32, 32, 1024, 1024, 1024, 2048, 2048, 0, 128, 1, (128, 0, 0), (128, 0, 0), (128, 0, 0), (128, 0, 0)),
    (0, 16, 64, 64, 64, 48, 16, 48, 16, 0, 1024, 1, (1024, 0, 0), (1024, 0, 0), (1024, 0, 0), (1024, 0, 0)),
    (0, 16, 128, 128, 128, 40, 24, 64, 64, 0, 2048, 1, (2048, 0, 0), (2048, 0, 0), (2048, 0, 0), (2048, 0, 0)),
    (1, 16, 64, 64, 64, 64, 0, 64, 0, 0, 512, 1, (512, 0, 0), (512, 0, 0), (512, 0, 0), (512, 0, 0)),
    (1, 2, 16, 16, 512, 512, 512, 1024, 1024, 0, 4, 1, (4, 0, 0), (4, 0, 0), (4, 0, 0), (4, 0, 0)),
    (0, 16, 256, 256, 64, 64, 0, 64, 0, 1, 16384, 1, (16384, 2, 2), (16384, 0, 0), (16384, 2, 2), (16384, 2, 2)),
    (0, 16, 32, 32, 512, 512, 0, 512, 0, 1, 256, 1, (256, 0, 0), (256, 0, 0), (256, 0, 0), (256, 0, 0)),
]


def conv3x3_queries(lib):
    out = []
    for (dt, B, H, W, co, c0, c1, ld0, ld1, hb) in (r[:10] for r in CONV3X3_QUERIES):
        out.append([lib.s2s_conv3x3_stat_blocks(dt, B, H, W, co), lib.s2s_conv3x3_ksplit(dt, B, H, W, co, c0 + c1),
                    lib.s2s_conv3x3_stat_rows(dt, B, H, W, co, c0, c1, ld0, ld1, hb),
                    lib.s2s_conv3x3_staged(dt, B, H, W, co, c0, c1, ld0, ld1, co, 0),
                    lib.s2s_conv3x3_staged(dt, B, H, W, co, c0, c1, ld0, ld1, co, 1)])
    return out


def test_conv3x3_launch_plan_queries():
    """The queries a caller sizes stat_part and kwork with, and the staged-kernel query, over the production shapes and
    under each launch switch.  The switches are read once per process, so every setting but the default runs in a child."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    from stain2stain_amd import _native
    for k, env in enumerate(CONV3X3_QUERY_ENVS):
        want = [[r[10], r[11], *r[12 + k]] for r in CONV3X3_QUERIES]
        if not env:
            got = conv3x3_queries(_native.lib())
        else:
            code = ("import json, sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_native_cpu as t; "
                    "from stain2stain_amd import _native; print(json.dumps(t.conv3x3_queries(_native.lib())))")
            run = subprocess.run([sys.executable, "-c", code, ROOT, os.path.join(ROOT, "tests")], env={**os.environ, **env},
                                 capture_output=True, text=True, timeout=300)
            assert run.returncode == 0, run.stderr[-2000:]
            got = json.loads(run.stdout.strip().splitlines()[-1])
        bad = [(r[:10], g, w) for r, g, w in zip(CONV3X3_QUERIES, got, want) if g != w]
        assert not bad, (env, bad[:5])
