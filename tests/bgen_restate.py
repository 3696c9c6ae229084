"""NumPy restatement of the device BGEN walk (k_bgen_walk, regenie_amd/csrc/bgen_inflate.hip) over inflated layout-2 blocks: shared by
tests/test_bgen_device_gpu.py and tests/test_bgen_device_edges_gpu.py.  Integers throughout: every comparison against it is exact."""
import numpy as np


def expect(blocks, n_file, file_idx, ref_first, mask=None, coding=0):
    """blocks [nvar, 10 + 3 N] uint8 -> g16 rows, the exact sums and, with `mask` [P, n] (0 = missing for the trait), their per-trait parts.
    coding 1 / 2: the rows hold P(het) + P(hom) / P(hom) of the counted allele; the sums stay those of the dosage."""
    fi = np.arange(n_file) if file_idx is None else np.asarray(file_idx)
    miss = (blocks[:, 8:8 + n_file] & 0x80) != 0
    pr = blocks[:, 10 + n_file:10 + 3 * n_file].reshape(blocks.shape[0], n_file, 2).astype(np.int64)
    b0, b1 = pr[:, fi, 0], pr[:, fi, 1]
    ms = miss[:, fi]
    bx = np.where(b0 + b1 < 255, 255 - b0 - b1, 0) if ref_first else b0
    q = b1 + 2 * bx
    inf = 255 * (4 * bx + b1) - q * q
    obs = ~ms
    row = q if coding == 0 else (b1 + bx if coding == 1 else bx)
    out = {"g16": np.where(ms, 0xFFFF, row).astype(np.uint16), "sum_q": (q * obs).sum(axis=1), "sum_info": (inf * obs).sum(axis=1),
           "n_obs": obs.sum(axis=1), "max_q": np.where(obs, q, 0).max(axis=1)}
    if mask is not None:
        mm = (np.asarray(mask) == 0)                                  # [P, n]: missing for the trait
        out["sum_q_t"] = np.stack([((q * obs) * mm[p]).sum(axis=1) for p in range(mm.shape[0])], axis=1)
        out["sum_info_t"] = np.stack([((inf * obs) * mm[p]).sum(axis=1) for p in range(mm.shape[0])], axis=1)
        out["n_obs_t"] = np.stack([(obs * mm[p]).sum(axis=1) for p in range(mm.shape[0])], axis=1)
    return out


def check(res, want):
    assert (res["status"] == 0).all(), res["status"]
    for k, v in want.items():
        assert np.array_equal(res[k], v), k
    assert (res["g16_pad"] == 0).all()
