"""EvalAccumulator on CPU: per-rank batch-size-weighted sums, one gloo all-reduce (world_size = 2) to the global
weighted mean over every rank's batches, reset()."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_single_process_weighted_mean_and_reset():
    from stain2stain_amd import EvalAccumulator
    acc = EvalAccumulator()
    acc.add({"loss": torch.tensor(1.0), "iou": torch.tensor(0.5)}, 2)
    acc.add({"loss": torch.tensor(4.0), "iou": torch.tensor(0.25)}, 6)
    out = acc.compute()
    assert sorted(out) == ["iou", "loss"]
    assert abs(float(out["loss"]) - (2 * 1.0 + 6 * 4.0) / 8) < 1e-6
    assert abs(float(out["iou"]) - (2 * 0.5 + 6 * 0.25) / 8) < 1e-6
    acc.reset()
    acc.add({"loss": torch.tensor(3.0), "iou": torch.tensor(1.0)}, 5)
    out = acc.compute()
    assert float(out["loss"]) == 3.0 and float(out["iou"]) == 1.0
    try:
        acc.add({"loss": torch.tensor(3.0)}, 1)
        raise AssertionError("a missing key must raise")
    except KeyError:
        pass


def test_inference_mode_then_reset():
    """Batches added under torch.inference_mode() (Lightning's validation loop) leave a buffer reset() can clear."""
    from stain2stain_amd import EvalAccumulator
    acc = EvalAccumulator()
    with torch.inference_mode():
        acc.add({"loss": torch.tensor(2.0)}, 3)
    acc.reset()
    acc.add({"loss": torch.tensor(5.0)}, 1)
    assert float(acc.compute()["loss"]) == 5.0


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


# rank -> [(batch size, loss, iou)]: different batch counts and sizes per rank
_BATCHES = {0: [(4, 1.0, 0.25), (3, 2.0, 0.5), (1, 7.0, 1.0)],
            1: [(2, 3.0, 0.75)]}


def _expect(key_idx):
    num = sum(b * v[key_idx] for r in _BATCHES.values() for b, *v in r)
    den = sum(b for r in _BATCHES.values() for b, *_ in r)
    return num / den


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from stain2stain_amd import EvalAccumulator
    acc = EvalAccumulator()
    for b, loss, iou in _BATCHES[rank]:
        acc.add({"loss": torch.tensor(loss), "iou": torch.tensor(iou)}, b)
    out = acc.compute()
    ok = abs(float(out["loss"]) - _expect(0)) < 1e-6 and abs(float(out["iou"]) - _expect(1)) < 1e-6
    # compute() leaves the local sums alone (a second call gives the same), reset() clears them
    again = acc.compute()
    ok = ok and float(again["loss"]) == float(out["loss"])
    acc.reset()
    acc.add({"loss": torch.tensor(float(rank + 1)), "iou": torch.tensor(0.0)}, 1 + rank)
    out = acc.compute()
    ok = ok and abs(float(out["loss"]) - (1 * 1.0 + 2 * 2.0) / 3) < 1e-6
    # a rank without batches takes part through keys given up front
    idle = EvalAccumulator(keys=["loss"], device="cpu")
    if rank == 0:
        idle.add({"loss": torch.tensor(6.0)}, 2)
    ok = ok and float(idle.compute()["loss"]) == 6.0
    q.put((rank, ok))
    dist.destroy_process_group()


def test_world2_global_weighted_mean():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert res == {0: True, 1: True}
