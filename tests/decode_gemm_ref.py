"""Float64 reference of one decode-sized GEMM launch, described by the fields of mt3_gemm_view (mt3_op_gemm_decode),
written from the rules in mt3_amd/csrc/kernels.h (GemmArgs) and include/mt3_hip.h, in torch on whatever device the
operands live on.  The operands are taken as they are (already rounded to the compute type); an f32 A operand
(a_is_f32) is rounded to the compute type first, as the kernel does while it stages it.

  row scale        rs = 1 (norm 0) | rsqrt(mean(A_f32^2) + 1e-6) from the f32 rows (norm 1)
                      | rsqrt(sum(a_ss[row]) / K + 1e-6) from the partial sums that arrive with the rows (norm 2)
  primary region   P = rs * (A . Wt[:n1]^T), n1 = n_split with a second product, else N
                   STORE, F32: P.   RESID: out + P.
                   GEGLU: weight rows interleaved in 16s -- rows [32q, 32q + 16) are gate columns 16q .., rows
                   [32q + 16, 32q + 32) linear columns 16q .. -- and out[:, 16q + c] = gelu_tanh(gate) * linear
  by-products      of the updated RESID rows: their rounding to the compute type (out_ct) and the sums of squares of their
                   16-column groups (out_ss)
  second product   S = A . Wt[n_split:N]^T: NO row scale, no activation.  STORE / GEGLU store it, RESID adds it to what is
                   there; row r lives at out2 + r * ld2, and only the first `side width` columns of a row are touched
                   (GEGLU: the weight rows are padded to whole 64-column tiles, the side width is ld2)

Also here: the operands the GPU tests feed the launches with (their conditions are checked on the CPU in
tests/test_decode_gemm_ref.py).
"""
import math

import torch

EPI_STORE, EPI_RESID, EPI_GEGLU, EPI_F32 = 0, 1, 2, 4            # MT3_EPI_* (include/mt3_hip.h)
PAD_WEIGHT = 1.0e30                                               # what the padding rows of a GEGLU side weight hold


def gelu_tanh(x):
    return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def row_scales(norm, A, a_ss, K):
    """1 / rms per row, float64 [M][1]"""
    M = A.shape[0]
    if norm == 0:
        return torch.ones(M, 1, dtype=torch.float64, device=A.device)
    if norm == 1:
        return torch.rsqrt((A[:, :K].double() ** 2).mean(-1, keepdim=True) + 1e-6)
    return torch.rsqrt(a_ss.double().sum(-1, keepdim=True) / K + 1e-6)


def interleave16(gate_t, lin_t):
    """gate_t, lin_t [F][K] (output-major) -> [2F][K] in alternating groups of 16 rows"""
    F, K = gate_t.shape
    w = torch.empty(2 * F, K, dtype=gate_t.dtype, device=gate_t.device)
    w.view(F // 16, 2, 16, K)[:, 0] = gate_t.reshape(F // 16, 16, K)
    w.view(F // 16, 2, 16, K)[:, 1] = lin_t.reshape(F // 16, 16, K)
    return w


def evaluate(*, A, Wt, M, N, K, epilogue, ct, norm=0, a_is_f32=False, a_ss=None, out=None, n_split=0, ld2=0, side=None):
    """One launch -> (primary float64 [M][width], second product float64 [M][side width] or None).
    A [M][>= K]; Wt [N][K]; a_ss [M][K / 16] (norm 2); out: the f32 rows [M][n1] a RESID launch adds to; n_split > 0: the
    launch carries a second product (out2 non-NULL in the view); side: what its region holds before a RESID launch
    [M][N - n_split]; ld2: GEGLU only, the side width (0: N - n_split)."""
    rs = row_scales(norm, A[:M], a_ss[:M] if a_ss is not None else None, K)
    a = A[:M, :K]
    a = (a.to(ct) if a_is_f32 else a).double()
    w = Wt[:N].double()
    n1 = n_split if n_split else N
    P = (a @ w[:n1].T) * rs
    if epilogue in (EPI_STORE, EPI_F32):
        primary = P
    elif epilogue == EPI_RESID:
        primary = out[:M, :n1].double() + P
    elif epilogue == EPI_GEGLU:
        g = P.view(M, n1 // 32, 2, 16)
        primary = (gelu_tanh(g[:, :, 0]) * g[:, :, 1]).reshape(M, n1 // 2)
    else:
        raise ValueError("no decode-sized launch has epilogue %d" % epilogue)
    if not n_split:
        return primary, None
    S = a @ w[n_split:].T                                         # unscaled: rs belongs to the primary region alone
    if epilogue == EPI_GEGLU:
        S = S[:, :(ld2 if ld2 else N - n_split)]
    elif epilogue == EPI_RESID:
        S = side[:M, :N - n_split].double() + S
    elif epilogue != EPI_STORE:
        raise ValueError("epilogue %d has no second product" % epilogue)
    return primary, S


def by_products(rows, ct):
    """f32 rows [M][W] -> (their rounding to the compute type, float64 sums of squares of their 16-column groups)"""
    M, W = rows.shape
    return rows.to(ct), (rows.double() ** 2).view(M, W // 16, 16).sum(-1)


def placed(before, value, col0=0):
    """The buffer [R][ld] a correct launch leaves: `before` with rows [0, M) x columns [col0, col0 + width) replaced by
    `value` [M][width] (cast to the buffer's type) -- everything else, padding columns and guard rows, as it was."""
    after = before.clone()
    M, W = value.shape
    after[:M, col0:col0 + W] = value.to(before.dtype)
    return after


def untouched(after, before, M, col0, width):
    """True if `after` equals `before` bit for bit outside rows [0, M) x columns [col0, col0 + width)"""
    bits = {2: torch.int16, 4: torch.int32}[before.element_size()]
    diff = after.view(bits) != before.view(bits)
    diff[:M, col0:col0 + width] = False
    return not bool(diff.any())


def rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))


def worst_row(got, ref):
    d = (got.double() - ref.double()).norm(dim=1) / ref.double().norm(dim=1).clamp_min(1e-30)
    return float(d.max())


# ------------------------------------------------------------------------------------------------- operands of the cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def residual_rows(M, K, seed):
    """f32 rows [M][K] with an rms between 12 and 42, so that a 1/rms applied where it does not belong (or left out where
    it does) is an error of order one"""
    g = _gen(seed)
    return torch.randn(M, K, generator=g) * (12 + 30 * torch.rand(M, 1, generator=g))


def partial_sums(x_ct):
    """the sums of squares of the 16-column groups of the rows a norm-2 launch reads, f32 [M][K / 16]"""
    M, K = x_ct.shape
    return (x_ct.double() ** 2).view(M, K // 16, 16).sum(-1).float()


def activations(M, K, seed, ct):
    """the compute-type A operand of a residual add (an attention output, a GEGLU output): unit normals"""
    return torch.randn(M, K, generator=_gen(seed)).to(ct)


def weight(N, K, seed, ct):
    """[N][K] output-major, unit-variance products; independent entries: nothing about it is symmetric"""
    return (torch.randn(N, K, generator=_gen(seed)) / math.sqrt(K)).to(ct)


def geglu_weight(F, K, seed, ct, n_side=0):
    """-> (Wt [2F + 64 * ceil(n_side / 64)][K]: gate / linear rows interleaved in 16s, then n_side side rows, then padding
    rows that hold PAD_WEIGHT; gate_t [F][K]; lin_t [F][K]; side_t [n_side][K])"""
    gate_t, lin_t = weight(F, K, seed, ct), weight(F, K, seed + 1, ct)
    side_t = weight(n_side, K, seed + 2, ct) if n_side else torch.empty(0, K, dtype=ct)
    pad = (n_side + 63) // 64 * 64
    w = torch.full((2 * F + pad, K), PAD_WEIGHT).to(ct)
    w[:2 * F] = interleave16(gate_t, lin_t)
    w[2 * F:2 * F + n_side] = side_t
    return w, gate_t, lin_t, side_t
