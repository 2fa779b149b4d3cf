"""Measurement for DESIGN.md 3.30: rigid pre-alignment of a 4096^2 pair with a planted 2 degree rotation and a
150-pixel offset.

    python scripts/rigid_bench.py [--windows 9] [--inner 20] [--out profiles/rigid_bench.json] [--kernels N]

The pair is ``scripts/region_warp_bench.py``'s synthetic pair (a residual shift of (3, -5) pixels stays in it); its target
is then resampled through the inverse of the plant with ``rigid_warp`` itself.

Legs:  (a) ``structure_overview`` at downsample 16 next to ``structure_map(downsample=4)`` over the same bytes: both read
           3 B per pixel once; the rate is 3 N^2 bytes over the time
       (b) ``rigid_warp`` of the image at 0, 2 and 5 degrees next to ``warp_region`` with a constant field and
           ``shift_tiles``, all moving 3 B in and 3 B out per pixel
       (c) ``register_rigid`` as a whole and its parts: the two overviews, the launch that rotates the target's overview
           by every angle, and the search level (sums and pick) over the angles
       (d) ``align_regions`` next to ``register_region`` on the same pair (``register_region`` cannot align this pair: its
           time is that of the same local work without the rigid stage)

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``; the legs of one group
alternate window by window inside this process and the median over ``--windows`` rounds is reported ((c) and (d) always
run 3 rounds of 2 calls; the JSON records the counts of every group).  No pass mark is
set on any time.  Kernel times are not taken here: they come from a separate run under a kernel trace, once of the
whole script and once with ``--kernels 10`` (ten calls of every leg of (a) and (b) in turn and nothing else), grouped
with ``scripts/kernel_groups.py``.
Writes one JSON object to ``--out`` and prints it."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from region_warp_bench import CELL, N, RADIUS, synthetic_region_pair, window_ms  # noqa: E402
from stain2stain_amd import (align_regions, register_region, register_rigid, rigid_transform, rigid_warp,  # noqa: E402
                             rotation_table, shift_tiles, structure_map, structure_overview, warp_region)
from stain2stain_amd import registration, rigid  # noqa: E402

ANGLE, OFFSET = 2.0, (120, -90)                # |offset| = 150 pixels
DS, SEARCH_RADIUS = 16, 32


def inverse(T):
    c, s, ty, tx, Cy, Cx = T.tolist()
    return torch.tensor([c, -s, -((c * ty + s * tx + (1 << 23)) >> 24), -((-s * ty + c * tx + (1 << 23)) >> 24), Cy, Cx],
                        dtype=torch.int64)


def alternating_ms(legs, windows, inner):
    """{name: median ms per call}: one window of every leg per round, in turn."""
    times = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            times[k].append(window_ms(fn, inner))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rigid_bench.json"))
    ap.add_argument("--kernels", type=int, default=0, metavar="N",
                    help="for a run under a kernel trace: N calls of every leg of (a) and (b) in turn, nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("rigid_bench needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    src, tgt0 = synthetic_region_pair(dev, 1)
    plant = rigid_transform(ANGLE, OFFSET, shape=(N, N))
    tgt = rigid_warp(tgt0, inverse(plant))
    del tgt0

    found = register_rigid(src, tgt)
    T = found["transform"]
    G = N // CELL
    const_field = torch.tensor([16 * 3, -16 * 5], dtype=torch.int32, device=dev).repeat(G, G, 1)
    one_shift = torch.tensor([[3, -5]], dtype=torch.int32, device=dev)
    T_at = {a: rigid_transform(a, (3, -5), shape=(N, N)).to(dev) for a in (0.0, 2.0, 5.0)}

    # the parts of register_rigid, as it runs them
    angles = rigid._angle_list(5.0, 0.5, None, "rigid_bench")
    h = N // DS
    tables = [(c, s, 0, 0, h - 1, h - 1) for c, s in rotation_table(angles).tolist()]
    m = rigid._inset(tables, h, h)
    Tk = torch.tensor(tables, dtype=torch.int64).to(dev)
    a_map, b_map = structure_overview(src, DS), structure_overview(tgt, DS, stains="hdab")
    bk = rigid_warp(b_map, Tk, nearest=False, fill=0)
    ac = a_map[m:h - m, m:h - m].expand(len(angles), h - 2 * m, h - 2 * m).contiguous()
    bc = bk[:, m:h - m, m:h - m].contiguous()

    groups = {
        "a": {"structure_overview_ds16": lambda: structure_overview(tgt, DS),
              "structure_map_ds4": lambda: structure_map(tgt[None], downsample=4)},
        "b": {"rigid_warp_0deg": lambda: rigid_warp(tgt, T_at[0.0]),
              "rigid_warp_2deg": lambda: rigid_warp(tgt, T_at[2.0]),
              "rigid_warp_5deg": lambda: rigid_warp(tgt, T_at[5.0]),
              "warp_region_constant_field": lambda: warp_region(tgt, const_field, CELL),
              "shift_tiles_one_launch": lambda: shift_tiles(tgt[None], one_shift)},
        "c": {"register_rigid": lambda: register_rigid(src, tgt),
              "two_overviews": lambda: (structure_overview(src, DS), structure_overview(tgt, DS, stains="hdab")),
              "rotate_all_angles": lambda: rigid_warp(b_map, Tk, nearest=False, fill=0),
              "search_level": lambda: registration._level(ac, bc, SEARCH_RADIUS, None, 1)},
        "d": {"align_regions": lambda: align_regions(src, tgt, CELL, radius=RADIUS),
              "register_region": lambda: register_region(src, tgt, CELL, radius=RADIUS)},
    }
    if args.kernels:                                               # the three rigid_warp legs differ in duration only:
        for g in ("a", "b"):                                       # scripts/kernel_groups.py name:N tells them apart
            for fn in groups[g].values():
                for _ in range(args.kernels):
                    fn()
        torch.cuda.synchronize()
        return
    for legs in groups.values():                                   # warm up: code objects, allocator
        for fn in legs.values():
            for _ in range(2):
                fn()
    torch.cuda.synchronize()

    out = {"shape": {"region": N, "cell": CELL, "downsample": DS, "overview": h, "angles": len(angles), "inset": m,
                     "search_radius": SEARCH_RADIUS, "local_radius": RADIUS},
           "planted": {"angle": ANGLE, "offset": list(OFFSET), "transform": plant.tolist()},
           "found": {"angle": float(found["angle"]), "transform": T.tolist(), "score": round(float(found["score"]), 4),
                     "angle_margin": round(float(found["angle_margin"]), 4), "valid": int(found["valid"])},
           "identity_equals_shift_tiles": bool(torch.equal(groups["b"]["rigid_warp_0deg"](),
                                                            groups["b"]["shift_tiles_one_launch"]()[0])),
           "identity_equals_warp_region": bool(torch.equal(groups["b"]["rigid_warp_0deg"](),
                                                           groups["b"]["warp_region_constant_field"]()))}
    aligned = align_regions(src, tgt, CELL, radius=RADIUS)
    out["align_regions_cells_kept"] = int(aligned["stats"][0])
    ms = {}
    rounds = {g: (3, 2) if g in ("c", "d") else (args.windows, args.inner) for g in groups}    # the slow groups: fewer
    for g, legs in groups.items():
        ms[g] = alternating_ms(legs, *rounds[g])
    out["windows_and_inner_by_group"] = {g: list(r) for g, r in rounds.items()}
    out["ms_per_call"] = {g: {k: round(v, 5) for k, v in legs.items()} for g, legs in ms.items()}
    out["a_read_GB_per_s"] = {k: round(3 * N * N / v * 1e-6, 1) for k, v in ms["a"].items()}
    out["b_in_plus_out_GB_per_s"] = {k: round(6 * N * N / v * 1e-6, 1) for k, v in ms["b"].items()}
    out["b_rigid_0deg_over_warp_region"] = round(ms["b"]["rigid_warp_0deg"] / ms["b"]["warp_region_constant_field"], 3)
    out["b_rigid_0deg_over_shift_tiles"] = round(ms["b"]["rigid_warp_0deg"] / ms["b"]["shift_tiles_one_launch"], 3)
    whole = ms["c"]["register_rigid"]
    out["c_share_of_register_rigid"] = {k: round(v / whole, 3) for k, v in ms["c"].items() if k != "register_rigid"}
    out["d_align_over_register_region"] = round(ms["d"]["align_regions"] / ms["d"]["register_region"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
