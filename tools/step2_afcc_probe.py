#!/usr/bin/env python
"""Times the two `--af-cc` entries of the Step-2 library (rg_s2_case_counts_packed, rg_s2_case_sums_int; csrc/step2_group.hip) on device rows:
kernel time per block from the library's own events (rg_s2_last_kernel_ms), the bytes the kernel must read and the share of the HBM bandwidth
that implies.  Default shape: 500,000 samples, 10 traits, blocks of 1,000 variants, with and without a male group set (one launch over both sets).

  python tools/step2_afcc_probe.py [--n 500000] [--traits 10] [--bs 1000] [--reps 20] [--hbm-gbs 8000]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, s2, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        fn()
        ms.append(s2.lib.rg_s2_last_kernel_ms(s2.h))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--traits", type=int, default=10)
    ap.add_argument("--bs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the bandwidth the shares are quoted against (GB/s)")
    a = ap.parse_args()
    import torch
    from regenie_amd.step2 import Step2QT
    n, P, bs = a.n, a.traits, a.bs
    rng = np.random.default_rng(1)
    masks = (rng.random((P, n)) > 0.05).astype(np.uint8)
    is_case = (rng.random((P, n)) < 0.2).astype(np.uint8)
    member = (rng.random(n) < 0.5).astype(np.uint8)
    ldb = (n + 3) // 4
    ldb = (ldb + 3) // 4 * 4
    rows = torch.from_numpy(rng.integers(0, 256, size=(bs, ldb), dtype=np.uint8)).cuda()
    ld16 = (n + 7) // 8 * 8
    G = rng.integers(0, 511, size=(bs, ld16), dtype=np.uint16)                      # 8-bit .bgen dosages (units of 1 / 255)
    G[rng.random((bs, ld16)) < 0.01] = 0xFFFF
    Gd = torch.from_numpy(G.view(np.int16)).cuda()
    nw = (n + 15) // 16
    out = {"n": n, "traits": P, "bs": bs, "hbm_gbs": a.hbm_gbs, "device": torch.cuda.get_device_name(0)}
    with Step2QT(n, 3, P) as s2:
        for tag, group in (("cases", False), ("cases+group", True)):
            s2.set_group(member if group else None, mask=masks if group else None)
            s2.set_cases(is_case, mask=masks)
            npl = P + (1 + P if group else 0)
            chunks = (npl + 7) // 8
            for name, fn, row_bytes in (("counts_packed", lambda: s2.case_counts(rows), ldb), ("sums_int", lambda: s2.case_sums_int(Gd), 2 * ld16)):
                t = timed(fn, s2, a.reps)
                once = bs * row_bytes + npl * nw * 4                                  # every row and every plane read once
                issued = bs * (chunks * row_bytes + npl * nw * 4)                     # what the workgroups ask for: a row per chunk of 8 planes, the planes per row
                t.update(planes=npl, plane_chunks=chunks, bytes_min=once, bytes_issued=issued,
                         gbs_min=once / t["median_ms"] / 1e6, share_of_hbm=once / t["median_ms"] / 1e6 / a.hbm_gbs,
                         gbs_issued=issued / t["median_ms"] / 1e6)
                out["%s/%s" % (tag, name)] = t
        # the group entry's one-sample-at-a-time kernel on the same rows, for comparison
        s2.set_cases(None)
        s2.set_group(member, mask=masks)
        out["group/sums_int (k_s2_group_sums_int)"] = timed(lambda: s2.group_sums_int(Gd), s2, a.reps)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
