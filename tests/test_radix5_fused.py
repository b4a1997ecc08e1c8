"""The FMA-fused 5-point butterfly of the N-point row pass (csrc/bds_acq_pfa.h: pk_radix5_tail, pk_radix5, pk_radix5_tw_k,
pk_radix25), restated in NumPy operation for operation -- one line per packed instruction, a fused multiply-add as one float64
multiply-add rounded once to the working type -- against the direct DFT sum, inverse direction (W = exp(+2 pi j / n)), which is
the only one the search uses.  float64: 1e-12 of the largest output; float32 inputs, constants and arithmetic: 1e-6.
(The operand-modifier bits of the instructions themselves are checked on the device: tests/test_butterflies5_gpu.py.)"""
import numpy as np
import pytest

KQ, KR5, KR, S1 = 0.25, 0.5590169943749475, 0.6180339887498949, 0.9510565162951535


class Pk:
    """Arithmetic on (re, im) pairs in one working type."""

    def __init__(self, dtype):
        self.t = dtype

    def fma(self, a, b, c):  # per half: a b + c, rounded once
        return self.t(np.float64(a) * np.float64(b) + np.float64(c))

    def add(self, a, b):
        return (self.t(a[0] + b[0]), self.t(a[1] + b[1]))

    def sub(self, a, b):
        return (self.t(a[0] - b[0]), self.t(a[1] - b[1]))

    def axpy(self, k, v, a):  # a + k v, k real (k negative: a - |k| v)
        k = self.t(k)
        return (self.fma(k, v[0], a[0]), self.fma(k, v[1], a[1]))

    def addjk(self, a, u, k):  # pk_addjk: a + j k u
        k = self.t(k)
        return (self.fma(-u[1], k, a[0]), self.fma(u[0], k, a[1]))

    def subjk(self, a, u, k):  # pk_subjk: a - j k u
        k = self.t(k)
        return (self.fma(u[1], k, a[0]), self.fma(-u[0], k, a[1]))

    def twice_minus(self, a, b):  # pk_twice_minus: 2 a - b
        return (self.fma(a[0], 2.0, -b[0]), self.fma(a[1], 2.0, -b[1]))

    def cmul_k(self, a, w):  # pk_cmul_k: v_pk_mul (a.x a.x)(w.x w.y), v_pk_fma (a.y a.y)(-w.y w.x) + .
        w = (self.t(w.real), self.t(w.imag))
        t = (self.t(a[0] * w[0]), self.t(a[0] * w[1]))
        return (self.fma(-a[1], w[1], t[0]), self.fma(a[1], w[0], t[1]))

    def bf2w_k(self, a, b, w):  # pk_bf2w_k: (a + w b, a - w b) = (p, 2 a - p)
        w = (self.t(w.real), self.t(w.imag))
        t = (self.fma(b[0], w[0], a[0]), self.fma(b[1], w[0], a[1]))
        p = (self.fma(-b[1], w[1], t[0]), self.fma(b[0], w[1], t[1]))
        return p, self.twice_minus(a, p)


def radix5_tail(P, x0, t1, t2, t3, t4):
    a, b = P.add(t1, t2), P.sub(t1, t2)
    m = P.axpy(-KQ, a, x0)
    m1, m2 = P.axpy(KR5, b, m), P.axpy(-KR5, b, m)
    u1 = P.axpy(KR, t4, t3)
    u2 = (P.fma(P.t(KR), t3[0], -t4[0]), P.fma(P.t(KR), t3[1], -t4[1]))
    y0 = P.add(x0, a)
    return [y0, P.addjk(m1, u1, S1), P.addjk(m2, u2, S1), P.subjk(m2, u2, S1), P.subjk(m1, u1, S1)]


def radix5(P, x):
    return radix5_tail(P, x[0], P.add(x[1], x[4]), P.add(x[2], x[3]), P.sub(x[1], x[4]), P.sub(x[2], x[3]))


def radix5_tw(P, x, w):  # over x0, w[1] x1 .. w[4] x4
    t1, t3 = P.bf2w_k(P.cmul_k(x[1], w[1]), x[4], w[4])
    t2, t4 = P.bf2w_k(P.cmul_k(x[2], w[2]), x[3], w[3])
    return radix5_tail(P, x[0], t1, t2, t3, t4)


def w25(k):
    return np.exp(2j * np.pi * k / 25)


def slot25_index(s):
    return 5 * (s % 5) + s // 5


def radix25(P, x, summed=False):
    """x[q0 + 5 q1] -> slot p0 + 5 p1 holds Y[5 p0 + p1]; summed: x[q0 + 15], x[q0 + 20] arrive as x2 + x3, x1 + x4."""
    x = list(x)
    for q0 in range(5):
        v = [x[q0 + 5 * q1] for q1 in range(5)]
        if summed:
            y = radix5_tail(P, v[0], v[4], v[3], P.twice_minus(v[1], v[4]), P.twice_minus(v[2], v[3]))
        else:
            y = radix5(P, v)
        for p1 in range(5):
            x[q0 + 5 * p1] = y[p1]
    x[0:5] = radix5(P, x[0:5])
    for p1 in range(1, 5):
        x[5 * p1:5 * p1 + 5] = radix5_tw(P, x[5 * p1:5 * p1 + 5], [w25(q0 * p1) for q0 in range(5)])
    return x


def to_pairs(P, z):  # complex [n][cases] -> list of n (re, im) pairs
    return [(P.t(row.real), P.t(row.imag)) for row in z]


def to_complex(y):
    return np.array([np.asarray(a, np.float64) + 1j * np.asarray(b, np.float64) for a, b in y])


def dft(z, n):  # inverse direction, direct sum in float64
    k = np.arange(n)
    return np.exp(2j * np.pi * np.outer(k, k) / n) @ z


def cases(n, dtype, seed):
    rng = np.random.default_rng(seed)
    z = np.concatenate([rng.standard_normal((n, 16)) + 1j * rng.standard_normal((n, 16)), np.eye(n) * (0.6 - 0.8j), np.ones((n, 1)) * (1 + 0j)], axis=1)
    if dtype is np.float32:  # the inputs are float32 values: the reference transforms those
        z = z.real.astype(np.float32).astype(np.float64) + 1j * z.imag.astype(np.float32).astype(np.float64)
    return z


BOUND = {np.float64: 1e-12, np.float32: 1e-6}


def rel_err(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_radix5(dtype):
    P = Pk(dtype)
    z = cases(5, dtype, 1)
    assert rel_err(to_complex(radix5(P, to_pairs(P, z))), dft(z, 5)) < BOUND[dtype]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("p1", [1, 2, 3, 4])
def test_twiddled_radix5(dtype, p1):
    P = Pk(dtype)
    z = cases(5, dtype, 2 + p1)
    w = np.array([w25(q0 * p1) for q0 in range(5)])
    got = to_complex(radix5_tw(P, to_pairs(P, z), list(w)))
    assert rel_err(got, dft(w[:, None] * z, 5)) < BOUND[dtype]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("summed", [False, True])
def test_radix25_slots(dtype, summed):
    P = Pk(dtype)
    z = cases(25, dtype, 7)
    x = to_pairs(P, z)
    if summed:  # what the row pass hands over: the sums formed in the working type
        for q0 in range(5):
            x[q0 + 20], x[q0 + 15] = P.add(x[q0 + 5], x[q0 + 20]), P.add(x[q0 + 10], x[q0 + 15])
    got = to_complex(radix25(P, x, summed))
    ref = dft(z, 25)[[slot25_index(s) for s in range(25)]]
    assert rel_err(got, ref) < BOUND[dtype]
    assert sorted(slot25_index(s) for s in range(25)) == list(range(25))
