"""NumPy statement of the CONTRACT of the stratified resampling kernel (include/aesmc_hip.h,
aesmc_resample_step_stratified), written independently of the kernel's parallel structure — what the tests hold the
HIP result to, exactly.

The CDF is the systematic contract's, operation for operation (float64 `exp(row - max)`, sequential `cumsum`, division
by the last entry; NaN rows and rows without a finite maximum give the index K and a flag bit): with every uniform of a
row equal, the result IS the systematic contract's, which tests/test_stratified_contract.py pins against the suite's
oracle.  (This package never imports the oracle — tests/test_library.py — so the few lines are restated here.)
"""
import numpy as np

FLAG_NAN_LOG_WEIGHT = 1
FLAG_DEGENERATE_ROW = 2

# the largest float64 below 1: u + (K - 1) can round up to K, i.e. to the position 1.0, which lies in no stratum
BELOW_ONE = np.nextafter(np.float64(1.0), np.float64(0.0))


def stratified_ancestor_index(log_w, u):
    """log_w [B,K] float32/float64, u [B,K] float64 in [0, 1) -> (idx int64 [B,K], flags).

        c[j]     = cumsum(exp(log_w[b] - max))[j] / cumsum(...)[K-1]            (float64)
        pos[k]   = min((u[b,k] + k) / K, nextafter(1, 0))                       (float64: sum, division, clamp)
        idx[b,k] = #{ j : c[j] <= pos[k] }

    One position per stratum [k/K, (k+1)/K], so idx is non-decreasing along k; with the clamp a row with a finite
    maximum never yields K (a position that rounded up to 1.0 selects the first particle whose CDF entry is 1.0, one of
    positive weight)."""
    log_w = np.asarray(log_w)
    B, K = log_w.shape
    u = np.asarray(u, dtype=np.float64)
    if u.shape != (B, K):
        raise ValueError("stratified resampling takes one uniform per particle: u must be [{}, {}], got {}".format(
            B, K, u.shape))
    idx = np.empty((B, K), dtype=np.int64)
    flags = 0
    strata = np.arange(0, K)
    for b in range(B):
        row = log_w[b]
        if np.isnan(row).any():
            flags |= FLAG_NAN_LOG_WEIGHT
            idx[b] = K
            continue
        m = row.max() if K else 0.0
        if not np.isfinite(m):
            flags |= FLAG_DEGENERATE_ROW
            idx[b] = K
            continue
        w = np.exp(row.astype(np.float64) - np.float64(m))
        c = np.cumsum(w)
        c = c / c[-1]
        pos = np.minimum((u[b] + strata) / K, BELOW_ONE)
        idx[b] = np.searchsorted(c, pos, side="right")
    return idx, flags


def children_end(idx):
    """child_end[b,k] = #{k' : idx[b,k'] <= k} (int32 [B,K]) — the by-product the resampling launches deliver."""
    idx = np.asarray(idx)
    B, K = idx.shape
    out = np.empty((B, K), dtype=np.int32)
    for b in range(B):
        out[b] = np.searchsorted(np.sort(idx[b]), np.arange(K), side="right")
    return out
