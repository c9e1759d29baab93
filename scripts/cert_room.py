"""The depth-64 certificate's room on the data of tests/test_gpu_multi_oracle.py's dimension sweep, on the CPU.

For generate_vectors(4100, d, 42), nlist 32, nprobe 8 and the 50 queries of seed 1337: the gap between the 10th
and the 64th exact score over a query's probed lists (float64 over the oracle's lists and probe ranking), beside
twice the refine certificate's error bound of a row of those lists (filter.hip refine_kernel, the IVF residual
form: A = |q - c_l| (L2) or |q| (IP), X = the list's largest residual):

    L2: c_bf u A X + c_err u (A + X)^2 + c_abs A + 2 t A X
    IP: (c_bf + c_err) u |q| X + c_abs |q| + t |q| X + c_err u |q| |c_l| + g |q| max|x|

with c_bf = filter_f16_cerr, c_err = 4 D + 64, c_abs = filter_f16_abs at sx = 1 (an over-estimate: the store's
scale is a larger power of two), t = 2^-36 sqrt(D), g = (D / 8 + 8) u, u = 2^-24, D the tile dimension.  A query
whose gap exceeds twice the bound is certified at depth 64 at the latest.

A one-off: the constants are restated here by hand from kernels.h (filter_f16_cerr, filter_f16_abs), engine.cpp
(filter_cerr) and filter.hip as they stood when the figures in the test's docstring were taken, and nothing
keeps them in step with the code.  Re-read those three places before trusting a new run.

    python scripts/cert_room.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle as O  # noqa: E402

U = 2.0 ** -24
CASES = [(d, 0) for d in (20, 100, 200, 512, 768, 800, 1024, 1530, 1536, 2048)] + [(100, 1), (768, 1), (2048, 1)]


def tile_dim(d):
    if d <= 128:
        return (d + 31) // 32 * 32
    return next(t for t in (256, 512, 768, 1024, 1536, 2048) if d <= t)


def room(d, metric, n=4100, nlist=32, nprobe=8, nq=50, k=10, depth=64):
    x = O.generate_vectors(n, d, 42)
    q = O.generate_vectors(nq, d, 1337)
    cents, assign = O.ivf_build(x, nlist, metric)
    D = tile_dim(d)
    c_bf = (8192.0 + 4.0 + 2.0 * D + 64.0 + 8192.0 + 64.0) * (2.0 if metric == 0 else 1.0)
    c_err = 4.0 * D + 64.0
    c_abs = 2.0 ** -25 * np.sqrt(D) * (2.0 if metric == 0 else 1.0)
    t = 2.0 ** -36 * np.sqrt(D)
    g = (D / 8.0 + 8.0) * U
    x64, c64 = x.astype(np.float64), cents.astype(np.float64)
    X = np.array([np.sqrt(((x64[assign == l] - c64[l]) ** 2).sum(1)).max() if (assign == l).any() else 0.0
                  for l in range(nlist)])
    Xf = np.array([np.sqrt((x64[assign == l] ** 2).sum(1)).max() if (assign == l).any() else 0.0
                   for l in range(nlist)])
    gaps, bounds = [], []
    for i in range(nq):
        probes = np.asarray(O.ivf_probe(q[i], cents, nprobe, metric))
        rows = x64[np.isin(assign, probes)]
        qi = q[i].astype(np.float64)
        s = -((rows - qi) ** 2).sum(1) if metric == 0 else rows @ qi
        s = np.sort(s)[::-1]
        assert len(s) >= depth
        gaps.append(s[k - 1] - s[depth - 1])
        if metric == 0:
            A = np.sqrt(((c64[probes] - qi) ** 2).sum(1))
            Xl = X[probes]
            el = c_bf * U * A * Xl + c_err * U * (A + Xl) ** 2 + c_abs * A + 2 * t * A * Xl
        else:
            qn = np.sqrt((qi ** 2).sum())
            cn = np.sqrt((c64[probes] ** 2).sum(1))
            Xl = X[probes]
            el = (c_bf + c_err) * U * qn * Xl + c_abs * qn + t * qn * Xl + c_err * U * qn * cn + g * qn * Xf[probes]
        bounds.append(2.0 * el.max())
    return min(gaps), max(bounds), int(sum(gp <= b for gp, b in zip(gaps, bounds)))


if __name__ == "__main__":
    for d, m in CASES:
        gap, b2, short = room(d, m)
        print(f"d={d:5d} {'L2' if m == 0 else 'IP'}: smallest gap {gap:.4g}, largest 2 x bound {b2:.4g}, "
              f"queries without room {short} of 50", flush=True)
