#!/usr/bin/env python
"""Step 2, counts restricted to a sample group (rg_s2_set_group; chromosome X outside the PAR regions): device time of rg_s2_group_counts_packed and
rg_s2_group_sums_int at 500,000 samples, 10 covariates, 10 phenotypes beside the score call of the same block, and the score call's own time on a
context with and without a group (alternating; a context without one launches nothing of this).  Bytes counted for the bandwidth figure: one read
of the rows plus the P + 1 bit planes.  Usage (GPU box): python tools/step2_group_probe.py [n]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from regenie_amd.step2 import Step2QT


def main(n=500_000, C=10, P=10):
    rng = np.random.default_rng(1)
    X = np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, C - 1))]))[0]
    mask = (rng.random((n, P)) > 0.05).astype(np.uint8)
    res = rng.normal(size=(n, P))
    res = (res - X @ (X.T @ res)) * mask
    member = (rng.random(n) < 0.5).astype(np.uint8)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(3)
    plane_bytes = (P + 1) * ((n + 15) // 16) * 4
    with Step2QT(n, C, P) as plain, Step2QT(n, C, P) as grp:
        for s2 in (plain, grp):
            s2.set_null(X.T, res.T, mask.T, np.ones(P))
        grp.set_group(member)
        for bs in (1024, 4096):
            rows = torch.randint(0, 256, (bs, (n + 3) // 4), dtype=torch.uint8, device=dev, generator=g)
            rows = (rows | ((rows & 0x55) & ~((rows >> 1) & 0x55)) << 1).to(torch.uint8)      # 01 -> 11: no missing call
            t = {"plain": [], "group": [], "counts": []}
            for _ in range(6):      # alternating
                t["plain"].append(plain.score_block_packed(rows)["kernel_ms"])
                t["group"].append(grp.score_block_packed(rows)["kernel_ms"])
                grp.group_counts(rows)
                t["counts"].append(grp.lib.rg_s2_last_kernel_ms(grp.h))
            med = {k: float(np.median(v[1:])) for k, v in t.items()}
            byt = bs * ((n + 3) // 4) + plane_bytes
            print("packed bs %5d: score call %.3f ms (no group) / %.3f ms (group set; runs %s / %s) | group counts %.3f ms = %.1f %% of the score call, %.0f GB/s of rows + planes"
                  % (bs, med["plain"], med["group"], " ".join("%.3f" % v for v in t["plain"][1:]), " ".join("%.3f" % v for v in t["group"][1:]),
                     med["counts"], 100 * med["counts"] / med["plain"], byt / med["counts"] / 1e6), flush=True)
        bs = 1024
        G = torch.randint(0, 511, (bs, n), dtype=torch.int16, device=dev, generator=g)
        ts, tc = [], []
        for _ in range(5):
            ts.append(grp.score_block_int(G, 255)["kernel_ms"])
            grp.group_sums_int(G)
            tc.append(grp.lib.rg_s2_last_kernel_ms(grp.h))
        a, b = float(np.median(ts[1:])), float(np.median(tc[1:]))
        print("uint16 bs %5d: score call %.3f ms | group sums %.3f ms = %.1f %% of the score call, %.0f GB/s of rows + planes"
              % (bs, a, b, 100 * b / a, (bs * n * 2 + plane_bytes) / b / 1e6), flush=True)


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:2]))
