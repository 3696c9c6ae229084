#!/usr/bin/env python3
"""Times the LD-matrix library (include/rg_ld.h) on synthetic hard calls: append (upload, row store, covariate contraction) and finish
(panel-pair Gram on the i8 matrix cores + fp64 epilogue + 16-bit quantisation), and prints the Gram kernel's integer operations per
second.  With --driver DIR it also writes a .bed of the same size there and times `regenie-amd --step 2 --compute-corr` on it, and
`oracle/_ref/regenie` on the same files when that binary exists (--ref-threads).

With --dosage SCALE the panels are random integer dosages in units of 1 / SCALE generated on the device (uniform on [0, 2 SCALE], --miss
of them missing) and appended in place through append_int; --driver then writes an 8-bit zlib BGEN of the same size (scale 255 only)
and times `--compute-corr --ld-dosages`.  The effective rate 2 * 128^2 * n * tiles / time counts one multiply-add per sample pair of
a tile whatever the number of digit planes: the figure to hold against an fp64 matrix-core Gram.

With --sparse THR every repetition also times the two routes to the sparse form of the unscaled matrix (`--skip-scaleG --sparse-thr THR`)
on the panels it holds: the device route, finish_sparse (Gram, diagonal rules, count pass, scan, write pass, the triplets to the host),
and the host route that was the only one before it, finish(COV_F64) (Gram, the 8 M^2-byte matrix to the host) followed by numpy
applying the diagonal rules and the same predicate row by row over the upper triangle.  Both routes repeat the Gram; its kernel time
is printed beside them.  The two entry counts must agree.

  python tools/ld_probe.py --n 200000 --M 4096 [--miss 0.01] [--bsize 1024] [--dosage SCALE] [--sparse THR] [--driver DIR --ref-threads 16]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sparse_routes(ld, thr, cov_form):
    """The device route and the host route to the sparse form at threshold thr, timed with a host clock (both end synchronised)."""
    t0 = time.perf_counter()
    sd, row, col, val = ld.finish_sparse(thr)
    t1 = time.perf_counter()
    gram_dev = ld.kernel_ms
    cov = ld.finish(cov_form)
    t2 = time.perf_counter()
    gram_host = ld.kernel_ms
    d = np.diag(cov).copy()      # print_ld's two diagonal rules, then the predicate of Data.cpp:4417-4418 row by row
    zero = (d < 0) & (np.abs(d) < ld.TOL)
    cov[zero, :] = 0
    cov[:, zero] = 0
    hsd = np.sqrt(np.maximum(np.where(zero, 0.0, d), ld.NUMTOL))
    hrow, hcol, hval = [], [], []
    for i in range(ld.M - 1):
        v = cov[i, i + 1:] / hsd[i] / hsd[i + 1:]
        k = np.nonzero(np.abs(v) >= thr)[0]
        if k.size:
            hrow.append(np.full(k.size, i, np.int32))
            hcol.append((k + i + 1).astype(np.int32))
            hval.append(v[k])
    hcount = int(sum(x.size for x in hrow))
    t3 = time.perf_counter()
    same = hcount == len(row) and (hcount == 0 or (np.array_equal(np.concatenate(hrow), row) and np.array_equal(np.concatenate(hcol), col)))
    return {"thr": thr, "entries": int(len(row)), "host_entries": hcount, "same_pairs": bool(same),
            "device_route_s": t1 - t0, "device_route_gram_ms": gram_dev,
            "host_route_s": t3 - t1, "host_route_cov_to_host_s": t2 - t1, "host_route_threshold_s": t3 - t2, "host_route_gram_ms": gram_host,
            "matrix_bytes": 8 * ld.M * ld.M, "triplet_bytes": 16 * int(len(row))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--C", type=int, default=3)
    ap.add_argument("--miss", type=float, default=0.01)
    ap.add_argument("--bsize", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dosage", type=int, default=0)
    ap.add_argument("--sparse", type=float, default=0.0)
    ap.add_argument("--driver", default=None)
    ap.add_argument("--ref-threads", type=int, default=16)
    ap.add_argument("--ref-timeout", type=int, default=600)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from regenie_amd.ld import COV_F64, R2_U16, LDMatrix
    n, M, nb = a.n, a.M, (a.n + 3) // 4
    rng = np.random.default_rng(1)
    X = np.linalg.qr(np.column_stack([np.ones(n), rng.normal(size=(n, a.C - 1))]))[0]
    g = torch.Generator(device="cuda").manual_seed(1)
    panels = []
    for p0 in range(0, M if a.dosage else 0, a.bsize):
        bs = min(a.bsize, M - p0)
        v = torch.randint(0, 2 * a.dosage + 1, (bs, n), device="cuda", generator=g, dtype=torch.int32)
        if a.miss > 0:
            v[torch.rand((bs, n), device="cuda", generator=g) < a.miss] = 0xFFFF
        panels.append(v.to(torch.int16).contiguous())      # (the 16 low bits: 0xFFFF and 2 * 16384 keep their pattern)
        del v
    for p0 in range(0, 0 if a.dosage else M, a.bsize):
        bs = min(a.bsize, M - p0)
        maf = torch.rand((bs, 1), device="cuda", generator=g) * 0.48 + 0.02
        u = torch.rand((bs, 4 * nb), device="cuda", generator=g)
        gt = (u < maf * maf).to(torch.uint8) + (u < 1 - (1 - maf) ** 2).to(torch.uint8)
        code = torch.where(gt == 2, 0, torch.where(gt == 1, 2, 3)).to(torch.uint8)
        if a.miss > 0:
            code[torch.rand((bs, 4 * nb), device="cuda", generator=g) < a.miss] = 1
        code[:, n:] = 0
        code = code.view(bs, nb, 4)
        panels.append((code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).contiguous().cpu().numpy())
        del u, gt, code
    res = {"n": n, "M": M, "C": a.C, "miss": a.miss, "bsize": a.bsize, "dosage_scale": a.dosage, "runs": []}
    nprod = 1 if not a.dosage else (2 if 2 * a.dosage <= 8127 else 3)      # digit planes of an operand
    for _ in range(a.reps):
        t0 = time.perf_counter()
        with LDMatrix(n, a.C, M) as ld:
            ld.set_basis(X.T)
            c0 = 0
            for rows in panels:
                if a.dosage:
                    ld.append_int(rows, np.arange(c0, c0 + rows.shape[0]), a.dosage)
                else:
                    ld.append(rows, np.arange(c0, c0 + rows.shape[0]))
                c0 += rows.shape[0]
            t1 = time.perf_counter()
            ld.finish(R2_U16)
            t2 = time.perf_counter()
            ms, tiles = ld.kernel_ms, ld.tiles
            sparse = sparse_routes(ld, a.sparse, COV_F64) if a.sparse > 0 else None
        ops = 2.0 * tiles * 128 * 128 * ((n + 63) // 64 * 64)
        run = {"append_s": t1 - t0, "finish_s": t2 - t1, "gram_ms": ms, "tiles": tiles, "gram_int_ops_per_s": ops / (ms * 1e-3)}
        if a.dosage:      # `tiles` counts 128 x 128 sums (A, B, Bt, D); an A tile runs nprod^2 plane products, a B tile nprod, a D tile one
            npair = ((M + 127) // 128) * ((M + 127) // 128 + 1) // 2
            rest = tiles - npair
            nd = npair if rest > 0 else 0      # with missing values in every tile: D per pair, B per pair and the mirrored B off the diagonal
            products = npair * nprod * nprod + (rest - nd) * nprod + nd
            run["gram_int_ops_per_s"] = 2.0 * products * 128 * 128 * ((n + 63) // 64 * 64) / (ms * 1e-3)
            run["effective_ops_per_s"] = 2.0 * tiles * 128 * 128 * n / (ms * 1e-3)
            run["plane_products"] = products
        if sparse:
            run["sparse"] = sparse
        res["runs"].append(run)
    if a.driver and a.dosage:
        import struct
        import zlib
        if a.dosage != 255:
            raise SystemExit("--driver with --dosage writes an 8-bit BGEN: scale 255")
        os.makedirs(a.driver, exist_ok=True)
        pre = os.path.join(a.driver, "ldprobe")
        with open(pre + ".bgen", "wb") as f:
            ids = b"".join(struct.pack("<H", len(s)) + s for s in (("%d_%d" % (i + 1, i + 1)).encode() for i in range(n)))
            sblock = struct.pack("<II", 8 + len(ids), n) + ids
            header = struct.pack("<III", 20, M, n) + b"bgen" + struct.pack("<I", 1 | (2 << 2) | (1 << 31))
            f.write(struct.pack("<I", len(header) + len(sblock)) + header + sblock)
            j = 0
            for rows in panels:
                q = rows.cpu().numpy().view(np.uint16)
                for r in q:      # dosage q = prob1 + 2 prob0 in units of 1 / 255: prob0 = q // 2, prob1 = q % 2 (+ 2 where prob0 allows, so that it is fractional)
                    miss = r == 0xFFFF
                    b0 = np.where(miss, 0, r // 2).astype(np.int64)
                    b1 = np.where(miss, 0, r % 2).astype(np.int64)
                    sh = (b0 > 0) & (b0 + b1 + 1 <= 255) & ~miss
                    b0 -= sh; b1 += 2 * sh
                    blk = struct.pack("<IHBB", n, 2, 2, 2) + np.where(miss, 0x82, 0x02).astype(np.uint8).tobytes() + bytes([0, 8])
                    blk += np.stack([b0, b1], axis=1).astype(np.uint8).tobytes()
                    z = zlib.compress(blk, 1)
                    rs = ("v%d" % (j + 1)).encode()
                    rec = struct.pack("<H", 0) + struct.pack("<H", len(rs)) + rs + struct.pack("<H", 1) + b"1" + struct.pack("<IH", j + 1, 2)
                    rec += struct.pack("<I", 1) + b"A" + struct.pack("<I", 1) + b"G" + struct.pack("<II", len(z) + 4, len(blk)) + z
                    f.write(rec)
                    j += 1
        with open(pre + ".covar", "w") as f:
            f.write("FID IID V1 V2\n")
            cv = rng.normal(size=(n, 2))
            for i in range(n):
                f.write("%d %d %.5f %.5f\n" % (i + 1, i + 1, cv[i, 0], cv[i, 1]))
        common = ["--step", "2", "--bgen", pre + ".bgen", "--covarFile", pre + ".covar", "--bsize", str(a.bsize), "--compute-corr"]
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")] + common + ["--ld-dosages", "--out", pre + "_amd"], capture_output=True, text=True)
        res["driver_wall_s"] = time.perf_counter() - t0
        res["driver_rc"] = r.returncode
        res["driver_tail"] = r.stdout[-400:]
        ref = os.path.join(ROOT, "oracle", "_ref", "regenie")
        if os.path.exists(ref):
            t0 = time.perf_counter()
            try:
                rr = subprocess.run([ref] + common + ["--threads", str(a.ref_threads), "--out", pre + "_ref"], capture_output=True, text=True, timeout=a.ref_timeout)
                res["reference_wall_s"], res["reference_rc"] = time.perf_counter() - t0, rr.returncode
                if rr.returncode == 0 and r.returncode == 0:
                    x = np.fromfile(pre + "_amd.corr", np.uint16)
                    y = np.fromfile(pre + "_ref.corr", np.uint16)
                    res["values_differing_from_reference"] = int((x != y).sum()) if x.shape == y.shape else -1
            except subprocess.TimeoutExpired:
                res["reference_wall_s"] = "> %d (stopped)" % a.ref_timeout
    elif a.driver:
        os.makedirs(a.driver, exist_ok=True)
        pre = os.path.join(a.driver, "ldprobe")
        with open(pre + ".bed", "wb") as f:
            f.write(bytes([0x6c, 0x1b, 0x01]))
            for rows in panels:
                f.write(rows.tobytes())
        with open(pre + ".bim", "w") as f:
            for j in range(M):
                f.write("1\tv%d\t0\t%d\tA\tG\n" % (j + 1, j + 1))
        with open(pre + ".fam", "w") as f:
            for i in range(n):
                f.write("%d %d 0 0 0 -9\n" % (i + 1, i + 1))
        with open(pre + ".covar", "w") as f:
            f.write("FID IID V1 V2\n")
            cv = rng.normal(size=(n, 2))
            for i in range(n):
                f.write("%d %d %.5f %.5f\n" % (i + 1, i + 1, cv[i, 0], cv[i, 1]))
        common = ["--step", "2", "--bed", pre, "--covarFile", pre + ".covar", "--bsize", str(a.bsize), "--compute-corr"]
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "regenie_amd", "bin", "regenie-amd")] + common + ["--out", pre + "_amd"], capture_output=True, text=True)
        res["driver_wall_s"] = time.perf_counter() - t0
        res["driver_rc"] = r.returncode
        ref = os.path.join(ROOT, "oracle", "_ref", "regenie")
        if os.path.exists(ref):
            t0 = time.perf_counter()
            try:
                rr = subprocess.run([ref] + common + ["--threads", str(a.ref_threads), "--out", pre + "_ref"], capture_output=True, text=True, timeout=a.ref_timeout)
                res["reference_wall_s"], res["reference_rc"] = time.perf_counter() - t0, rr.returncode
                if rr.returncode == 0 and r.returncode == 0:
                    x = np.fromfile(pre + "_amd.corr", np.uint16)
                    y = np.fromfile(pre + "_ref.corr", np.uint16)
                    res["values_differing_from_reference"] = int((x != y).sum()) if x.shape == y.shape else -1
            except subprocess.TimeoutExpired:
                res["reference_wall_s"] = "> %d (stopped)" % a.ref_timeout
    print(json.dumps(res))


if __name__ == "__main__":
    main()
