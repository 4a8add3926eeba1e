"""The arithmetic of the bf16 training attention core (csrc/train_attn16.hip, include/must3r_hip.h ``must3r_hip_train_attention_mode``) restated in plain torch
with its five rounding points -- Q, K, V, dO as operands; P as operand of P V and of P^T dO; dS as operand of dS K and dS^T Q -- and everything else in the
working dtype (fp64: what the formulas mean; fp32: the precision the kernels compute in).  With s = 1/8 and ^ = ``.to(torch.bfloat16)``:

    S = s (Q^ K^T^)          p = exp(S - m), l = sum p (unrounded)          O = (p^ V^) / l          lse = m + log l
    P = exp(S - lse)         delta = dO . O (unrounded dO)                  dV = P^T^ dO^            dP = dO^ V^T^
    dS = P (dP - delta)      dQ = s dS^ K^                                  dK = s dS^T^ Q^

``rounding=False`` removes the five roundings: the formulas of tests/attn_grad_ref.py, written out by hand instead of by autograd.  ``tiled=True`` runs the
forward as the kernel does, key tile by key tile of 64 with a running maximum (p is then rounded relative to the running maximum and the partial sums are
rescaled): another realisation of the same arithmetic, which stands in for the GPU in the host test of the parity rule.  ``defect`` plants what a wrong kernel
could do (``DEFECTS``).  ``keep``: per view ``None`` or a bool [nk] key mask on top of the table."""
import torch

from attn_grad_ref import HEAD, valid_mask

S = 0.125
DEFECTS = ("truncate_operand", "truncate_p", "l_rounded", "delta_rounded", "dk_no_scale", "dv_unrounded_p")


def rnd(t):
    """nearest even to bf16, NaN and inf kept, back in the dtype of t"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def chop(t):
    """truncation to bf16, back in the dtype of t"""
    return (t.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def _split(t, r0, n, heads):
    return t[r0:r0 + n].reshape(n, heads, HEAD).transpose(0, 1)


def _merge(t):
    return t.transpose(0, 1).reshape(t.shape[1], -1)


def core(case, dtype, rounding=True, defect=None, tiled=False, keep=None):
    """dict O, lse, dQ, dK, dV of a case of attn_grad_ref.make_case (q, k, v, dO, views, heads) in ``dtype``; lse [Rq, heads], -inf for a row without keys."""
    assert defect is None or defect in DEFECTS
    ident = lambda t: t
    r_op = ident if not rounding else chop if defect == "truncate_operand" else rnd
    r_p = ident if not rounding else chop if defect == "truncate_p" else rnd
    heads = case["heads"]
    Q, K, V, dO = (case[n].to(dtype) for n in ("q", "k", "v", "dO"))
    out = dict(O=torch.zeros_like(Q), lse=Q.new_full((Q.shape[0], heads), float("-inf")), dQ=torch.zeros_like(Q), dK=torch.zeros_like(K), dV=torch.zeros_like(V))
    for i, view in enumerate(case["views"]):
        q0, nq, k0, nk, _, _ = view
        valid = valid_mask(view)
        if keep is not None and keep[i] is not None:
            valid = valid & keep[i][:nk]
        if nq == 0 or nk == 0 or not bool(valid.any()):
            continue
        q, do, do_raw = r_op(_split(Q, q0, nq, heads)), r_op(_split(dO, q0, nq, heads)), _split(dO, q0, nq, heads)
        k, v = r_op(_split(K, k0, nk, heads)), r_op(_split(V, k0, nk, heads))
        s = (q @ k.transpose(1, 2)) * S
        s = s.masked_fill(~valid, float("-inf"))
        if tiled:
            m = s.new_full((heads, nq, 1), float("-inf"))
            l, acc = s.new_zeros((heads, nq, 1)), s.new_zeros((heads, nq, HEAD))
            for t0 in range(0, nk, 64):
                st = s[:, :, t0:t0 + 64]
                if not bool(valid[t0:t0 + 64].any()):
                    continue
                mn = torch.maximum(m, st.max(-1, keepdim=True).values)
                alpha = torch.exp(m - mn)
                p = torch.exp(st - mn)
                l = l * alpha + (r_p(p) if defect == "l_rounded" else p).sum(-1, keepdim=True)
                acc = acc * alpha + r_p(p) @ v[:, t0:t0 + 64]
                m = mn
        else:
            m = s.max(-1, keepdim=True).values
            p = torch.exp(s - m)
            l = (r_p(p) if defect == "l_rounded" else p).sum(-1, keepdim=True)
            acc = r_p(p) @ v
        o = acc / l
        lse = m + torch.log(l)
        P = torch.exp(s - lse)
        delta = ((r_op(do_raw) if defect == "delta_rounded" else do_raw) * o).sum(-1, keepdim=True)
        dv = (P if defect == "dv_unrounded_p" else r_p(P)).transpose(1, 2) @ do
        dS = r_p(P * (do @ v.transpose(1, 2) - delta))
        out["O"][q0:q0 + nq] = _merge(o)
        out["lse"][q0:q0 + nq] = lse[:, :, 0].t()
        out["dQ"][q0:q0 + nq] = _merge(dS @ k) * S
        out["dK"][k0:k0 + nk] += _merge(dS.transpose(1, 2) @ q) * (1.0 if defect == "dk_no_scale" else S)
        out["dV"][k0:k0 + nk] += _merge(dv)
    return out


def lse_bound(q, k):
    """The single-key check of tests/test_attn16_gpu.py: (exact s sum q^ k^ in fp64, (64 + 8) 2^-24 s sum |q^| |k^|) for q [nq, 64] and one key k [64]:
    63 additions, the two constant multiplications and their constants' roundings, and headroom."""
    q64, k64 = rnd(q).double(), rnd(k).double()
    return S * (q64 * k64).sum(-1), (64 + 8) * 2.0 ** -24 * S * (q64.abs() * k64.abs()).sum(-1)

