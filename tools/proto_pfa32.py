#!/usr/bin/env python3
"""NumPy model of the N-point search pair at 53 MS/s (csrc/bds_acq_pfa32.h), beside tools/proto_pfa53.py: N = 1 060 000 = 53 x 32 x 625.
    python tools/proto_pfa32.py maps     the Good-Thomas maps: 3-D transform == N-point transform, and the rotation of a Doppler bin
    python tools/proto_pfa32.py rows     the row pass's 625 = 25 x 25 split: lane j holds k3 = j + 25 q, lane t' ends with lags t' + 25 t''
    python tools/proto_pfa32.py cols     the column pass's 32-point stage as the lanes compute it: k2 = 8 m + 4 h + rr -> t2 = e + 2 tai + 16 h + 4 tbi
    python tools/proto_pfa32.py all
No hi-only bound pass is built (every output block is computed with hi + lo coefficients once), so there is no margin to model here;
for the record, the paper bound of such a pass at 32 x 53 = 1696 outputs per lag would be
2^-11 * 41.18 / (41.18 - sqrt(32) * 53 * 2^-11.5) = 4.9e-4 (41.18 = sqrt(1696))."""
import sys

import numpy as np

K1, K2, K3 = 53, 32, 625
N = K1 * K2 * K3


def lag_of(t1, t2, t3):
    return (t1 * (N // K1) + t2 * (N // K2) + t3 * (N // K3)) % N


def maps():
    rng = np.random.default_rng(0)
    k = np.arange(N)
    k_of = np.empty((K1, K2, K3), dtype=np.int64)
    k_of[k % K1, k % K2, k % K3] = k
    lag = lag_of(np.arange(K1)[:, None, None], np.arange(K2)[None, :, None], np.arange(K3)[None, None, :])
    assert np.array_equal(np.sort(k_of.ravel()), k) and np.array_equal(np.sort(lag.ravel()), k)
    Y = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    y3 = np.fft.ifftn(Y[k_of]) * N  # inverse 3-D transform of the CRT-ordered spectrum
    y1 = np.fft.ifft(Y) * N
    err = np.max(np.abs(y3 - y1[lag])) / np.max(np.abs(y1))
    print(f"maps: 3-D transform at lag_of(t1, t2, t3) vs the N-point transform: max error {err:.2e}")
    assert err < 1e-10
    for s in (1, 33, 53, 625, 640, 1252):  # the rotation of a bin: index k - s <-> every coordinate minus s, rows read from column -s
        X = np.roll(Y, s)[k_of]
        rot = Y[k_of][(np.arange(K1)[:, None, None] - s) % K1, (np.arange(K2)[None, :, None] - s) % K2, (np.arange(K3)[None, None, :] - s) % K3]
        assert np.array_equal(X, rot)
    print("maps: rotation by s = every coordinate minus s (s = 1 .. 1252): exact")


def rows():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(K3) + 1j * rng.standard_normal(K3)
    W = lambda n, d: np.exp(2j * np.pi * n / d)  # noqa: E731
    j, q, p = np.arange(25), np.arange(25), np.arange(25)
    a = np.einsum("jq,qp->jp", x[j[:, None] + 25 * q[None, :]], W(np.outer(q, p), 25)) * W(np.outer(j, p), K3)  # stage 1 + twiddle: a[j][p]
    X = np.einsum("jp,jt->pt", a, W(np.outer(j, np.arange(25)), 25))  # stage 2 in lane t' = p: X[t' + 25 t'']
    got = np.empty(K3, dtype=complex)
    got[p[:, None] + 25 * np.arange(25)[None, :]] = X
    err = np.max(np.abs(got - np.fft.ifft(x) * K3))
    print(f"rows: 25 x 25 split vs the 625-point inverse transform: max error {err:.2e}")
    assert err < 1e-9


def cols():
    rng = np.random.default_rng(2)
    z = rng.standard_normal(K2) + 1j * rng.standard_normal(K2)
    ref = np.fft.ifft(z) * K2
    W = lambda n, d: np.exp(2j * np.pi * n / d)  # noqa: E731
    got = np.full(K2, np.nan + 0j)
    S = {}
    for e in range(2):        # lane parity: the ta of the lane pair
        for h in range(2):    # 16-lane row: k2 = 8 m + 4 h + rr
            zz = np.array([[z[8 * m + 4 * h + rr] for rr in range(4)] for m in range(4)])  # [m][rr]
            for tai in range(2):
                ta = e + 2 * tai
                Zt = np.array([np.sum(zz[:, rr] * W(np.arange(4) * ta, 4)) * W((4 * h + rr) * ta, 32) for rr in range(4)])
                S[(e, h, tai)] = np.array([np.sum(Zt * W(np.arange(4) * tb, 8)) for tb in range(8)])
    for e in range(2):
        for tai in range(2):
            for h in range(2):      # after the swap: row h finishes tb = 4 h + tbi
                for tbi in range(4):
                    tb = 4 * h + tbi
                    y = S[(e, 0, tai)][tb] + (-1) ** tbi * S[(e, 1, tai)][tb]
                    t2 = e + 2 * tai + 16 * h + 4 * tbi
                    assert np.isnan(got[t2])
                    got[t2] = y
    err = np.max(np.abs(got - ref))
    print(f"cols: 32-point stage as the lanes compute it vs the 32-point inverse transform: max error {err:.2e}")
    assert err < 1e-12


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    for name, f in (("maps", maps), ("rows", rows), ("cols", cols)):
        if what in (name, "all"):
            f()
