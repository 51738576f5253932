"""numpy statements of the align_corners=True bilinear resize's taps and of its adjoint, shared by tests/test_resize_host.py (which
pins numpy_adjoint to torch's CPU autograd), tests/test_dwconv_geometry_host.py and tests/test_gpu_decoder_front.py."""
import math

import numpy as np


def make_taps(o, scale, n_in, T):
    """halo_softmax.hpp make_taps in dtype T"""
    f = T(scale) * T(o)
    i0 = min(int(f), n_in - 1)
    i1 = i0 + (1 if i0 < n_in - 1 else 0)
    l1 = T(f - T(i0))
    return i0, i1, T(T(1) - l1), l1


def scale_of(n_in, n_out, T):
    return T(n_in - 1) / T(n_out - 1) if n_out > 1 else T(0)


def weights(n_in, n_out, T):
    """(n_out, n_in): row o holds the weights of output coordinate o (both taps add where they coincide)"""
    A = np.zeros((n_out, n_in), dtype=T)
    s = scale_of(n_in, n_out, T)
    for o in range(n_out):
        i0, i1, l0, l1 = make_taps(o, s, n_in, T)
        A[o, i0] = T(A[o, i0] + l0)
        A[o, i1] = T(A[o, i1] + l1)
    return A


def numpy_adjoint(g, h, w):
    """grad_in[p, i, j] = sum_Y sum_X wy(Y, i) wx(X, j) g[p, Y, X] in g's dtype, ascending X inside a row, rows in ascending Y"""
    T = g.dtype.type
    P, H, W = g.shape
    Ay, Ax = weights(h, H, T), weights(w, W, T)
    out = np.zeros((P, h, w), dtype=T)
    for i in range(h):
        ys = np.nonzero(Ay[:, i])[0]
        for j in range(w):
            xs = np.nonzero(Ax[:, j])[0]
            acc = np.zeros(P, dtype=T)
            for Y in ys:
                r = np.zeros(P, dtype=T)
                for X in xs:
                    r = (r + Ax[X, j] * g[:, Y, X]).astype(T)
                acc = (acc + Ay[Y, i] * r).astype(T)
            out[:, i, j] = acc
    return out


def terms_bound(h, w, H, W):
    return (2 * math.ceil((H - 1) / max(h - 1, 1)) + 1) * (2 * math.ceil((W - 1) / max(w - 1, 1)) + 1)


def tap_matrices64(h, w, H, W):
    """(Ay (H, h), Ax (W, w)): the float32 tap weights of the device resize, as float64"""
    return weights(h, H, np.float32).astype(np.float64), weights(w, W, np.float32).astype(np.float64)


def resize64(a, H, W):
    """Ay a Ax^T in float64 over the last two axes: the resize with the float32 taps and exact arithmetic"""
    Ay, Ax = tap_matrices64(a.shape[-2], a.shape[-1], H, W)
    return np.einsum("Yi,...ij,Xj->...YX", Ay, np.asarray(a, dtype=np.float64), Ax)


def adjoint64(g, h, w):
    """Ay^T g Ax in float64 over the last two axes: the resize backward with the float32 taps and exact arithmetic"""
    Ay, Ax = tap_matrices64(h, w, g.shape[-2], g.shape[-1])
    return np.einsum("Yi,...YX,Xj->...ij", Ay, np.asarray(g, dtype=np.float64), Ax)
