"""Float64 restatement of the multi-resolution products (scarlet_amd/csrc/resample.hip), NumPy
only.  Layouts as the C interface takes them: A[C][n_a][Fy * Fx], Pt[Fx][Fx * n_b] with
Pt[x'][x * n_b + b] = P[x, b, x'], model[C][Fy][Fx], resid[C][n_a][n_b]."""

import numpy as np


def matmul64(A, B):
    """Batched product in float64 (BLAS); exact while every sum of |a||b| stays below 2^53."""
    return np.matmul(np.asarray(A, np.float64), np.asarray(B, np.float64))


def render64(A, Pt, model):
    """out[c, a, b] = sum_{y, x} A[c, a, (y, x)] sum_x' model[c, y, x'] Pt[x', (x, b)]"""
    C, Fy, Fx = model.shape
    n_b = Pt.shape[1] // Fx
    shifted = matmul64(model, Pt).reshape(C, Fy * Fx, n_b)
    return matmul64(A, shifted)


def adjoint64(A, Pt, resid):
    """g[c, y, x'] = sum_{x, b} (sum_a A[c, a, (y, x)] resid[c, a, b]) Pt[x', (x, b)]"""
    C, n_a, n_b = resid.shape
    Fx = Pt.shape[0]
    Fy = A.shape[2] // Fx
    back = matmul64(np.asarray(A, np.float64).transpose(0, 2, 1), resid)
    return matmul64(back.reshape(C, Fy, Fx * n_b), np.asarray(Pt, np.float64).T)


def circulant(kern):
    """Pt of the shift operator P[x, b, x'] = kern[b, (x - x') mod Fx]: what the reference's
    phase ramp amounts to, and what selects the spectral path."""
    n_b, Fx = kern.shape
    idx = (np.arange(Fx)[:, None] - np.arange(Fx)[None, :]) % Fx  # [x, x']
    P = kern[:, idx]  # [b, x, x']
    return np.ascontiguousarray(P.transpose(2, 1, 0).reshape(Fx, Fx * n_b))


def spectral_emulation(A, s, model=None, resid=None, table_dtype=np.float32):
    """The spectral algorithm of resample.hip's comment block on the CPU: the tables E (transforms
    of the operator rows), beta (weighted transforms of s_b over Fx) and Wx (cos, -sin) are made
    in float64 and rounded to ``table_dtype``, the two transforms along x are matrix products
    in ``table_dtype`` (as are their results Mh and Mbar and the stored Gbar), the sums over y,
    a, b and k are float64.  Returns (rendering or None, adjoint or None) in float64.

    With float32 tables the deviation from render64 / adjoint64 is the precision of the method
    itself, whatever device runs it; with float64 tables it is the same linear map to rounding."""
    C, Fy, Fx = (model.shape if model is not None else
                 (A.shape[0], A.shape[2] // s.shape[1], s.shape[1]))
    n_a, n_b = A.shape[1], s.shape[0]
    Kx = Fx // 2 + 1
    ctype = np.complex64 if table_dtype == np.float32 else np.complex128
    k = np.arange(Kx)
    w = np.where((k == 0) | (2 * k == Fx), 1.0, 2.0)
    E = np.fft.rfft(np.asarray(A, np.float64).reshape(C, n_a, Fy, Fx), axis=-1).astype(ctype)
    beta = (np.fft.rfft(np.asarray(s, np.float64), axis=-1) * w / Fx).astype(ctype)
    ang = 2.0 * np.pi * ((np.arange(Fx)[:, None] * k[None, :]) % Fx) / Fx
    Wx = np.empty((Fx, 2 * Kx), np.float64)
    Wx[:, 0::2], Wx[:, 1::2] = np.cos(ang), -np.sin(ang)
    Wx = Wx.astype(table_dtype)
    E64, beta64 = E.astype(np.complex128), beta.astype(np.complex128)
    out = grad = None
    if model is not None:
        Mh = np.matmul(np.asarray(model, table_dtype), Wx)  # [C][Fy][2 Kx]
        Mh = Mh[..., 0::2].astype(np.float64) + 1j * Mh[..., 1::2].astype(np.float64)
        G = np.einsum("cayk,cyk->cak", E64.conj(), Mh)
        out = np.einsum("bk,cak->cab", beta64, G).real
    if resid is not None:
        Gbar = np.einsum("cab,bk->cak", np.asarray(resid, np.float64), beta64.conj()).astype(ctype)
        Mbar = np.einsum("cak,cayk->cyk", Gbar.astype(np.complex128), E64).astype(ctype)
        flat = np.empty((C, Fy, 2 * Kx), table_dtype)
        flat[..., 0::2], flat[..., 1::2] = Mbar.real, Mbar.imag
        grad = np.matmul(flat, np.ascontiguousarray(Wx.T)).astype(np.float64)
    return out, grad
