"""Float64 NumPy restatement of the column-profile contract (include/radargrid_hip.h, ``rg_column_profile_f32``): echo-top
and echo-base height at a threshold and Greene & Clark's vertically integrated liquid, for one column at a time, in plain
loops over the levels.  A helper module (its name does not start with ``test_``): tests/test_column_profile_oracle.py pins
it to known answers, tests/test_gpu_column_profile.py compares the kernel with it.

Everything is written from the contract's text: the levels ``lo .. hi`` of the window only, float64 operations on the
float32 values in the stated association, one rounding to float32 at the end."""
import numpy as np

VIL_FACTOR = 3.44e-6


def _finite(v) -> bool:
    return bool(np.isfinite(v))


def echo_top_column(g, z, threshold, lo=0, hi=None, linear=True) -> np.float32:
    """``g``: the column's float32 values, ``z``: the float64 level heights; the window is ``lo .. hi`` inclusive."""
    g = np.asarray(g, dtype=np.float32)
    z = np.asarray(z, dtype=np.float64)
    hi = len(g) - 1 if hi is None else hi
    t = np.float64(threshold)
    k = None
    for lev in range(lo, hi + 1):                      # the highest level that reaches the threshold (NaN never does)
        if np.float64(g[lev]) >= t:
            k = lev
    if k is None:
        return np.float32(np.nan)
    if linear and k < hi and _finite(g[k]) and _finite(g[k + 1]):
        gk, gn = np.float64(g[k]), np.float64(g[k + 1])
        with np.errstate(all="ignore"):
            frac = (gk - t) / (gk - gn)
            return np.float32(z[k] + frac * (z[k + 1] - z[k]))
    return np.float32(z[k])


def echo_base_column(g, z, threshold, lo=0, hi=None, linear=True) -> np.float32:
    g = np.asarray(g, dtype=np.float32)
    z = np.asarray(z, dtype=np.float64)
    hi = len(g) - 1 if hi is None else hi
    t = np.float64(threshold)
    k = None
    for lev in range(lo, hi + 1):                      # the lowest level that reaches the threshold
        if np.float64(g[lev]) >= t:
            k = lev
            break
    if k is None:
        return np.float32(np.nan)
    if linear and k > lo and _finite(g[k]) and _finite(g[k - 1]):
        gk, gp = np.float64(g[k]), np.float64(g[k - 1])
        with np.errstate(all="ignore"):
            frac = (gk - t) / (gk - gp)
            return np.float32(z[k] - frac * (z[k] - z[k - 1]))
    return np.float32(z[k])


def vil_column(g, z, max_dbz=56.0, lo=0, hi=None) -> np.float32:
    g = np.asarray(g, dtype=np.float32)
    z = np.asarray(z, dtype=np.float64)
    hi = len(g) - 1 if hi is None else hi
    cap = np.float64(max_dbz)
    q = np.zeros(len(g), dtype=np.float64)
    seen = False
    with np.errstate(all="ignore"):
        for lev in range(lo, hi + 1):
            if np.isnan(g[lev]):
                q[lev] = 0.0
            else:
                seen = True
                q[lev] = np.float64(10.0) ** (min(np.float64(g[lev]), cap) / np.float64(10.0))
        if not seen:
            return np.float32(np.nan)
        total = np.float64(0.0)
        for lev in range(lo, hi):
            total = total + ((q[lev] + q[lev + 1]) / np.float64(2.0)) ** np.float64(4.0 / 7.0) * (z[lev + 1] - z[lev])
        return np.float32(np.float64(VIL_FACTOR) * total)


def _plane(fn, grid, z, *args, **kw) -> np.ndarray:
    grid = np.asarray(grid, dtype=np.float32)
    nz = grid.shape[0]
    cols = grid.reshape(nz, -1)
    out = np.empty(cols.shape[1], dtype=np.float32)
    for c in range(cols.shape[1]):
        out[c] = fn(cols[:, c], z, *args, **kw)
    return out.reshape(grid.shape[1:])


def echo_top(grid, z, threshold, lo=0, hi=None, linear=True) -> np.ndarray:
    """The plane of ``echo_top_column`` over a ``[nz, ...]`` grid."""
    return _plane(echo_top_column, grid, z, threshold, lo=lo, hi=hi, linear=linear)


def echo_base(grid, z, threshold, lo=0, hi=None, linear=True) -> np.ndarray:
    return _plane(echo_base_column, grid, z, threshold, lo=lo, hi=hi, linear=linear)


def vil(grid, z, max_dbz=56.0, lo=0, hi=None) -> np.ndarray:
    return _plane(vil_column, grid, z, max_dbz, lo=lo, hi=hi)
