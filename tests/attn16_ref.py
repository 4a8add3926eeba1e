"""The arithmetic of the bf16 training attention core (csrc/train_attn16.hip, include/must3r_hip.h ``must3r_hip_train_attention_mode``) restated in plain torch
with its five rounding points -- Q, K, V, dO as operands; P as operand of P V and of P^T dO; dS as operand of dS K and dS^T Q -- and everything else in the
working dtype (fp64: what the formulas mean; fp32: the precision the kernels compute in).  With s = 1/8 and ^ = ``.to(torch.bfloat16)``:

    S = s (Q^ K^T^)          p = exp(S - m), l = sum p (unrounded)          O = (p^ V^) / l          lse = m + log l
    P = exp(S - lse)         delta = dO . O (unrounded dO)                  dV = P^T^ dO^            dP = dO^ V^T^
    dS = P (dP - delta)      dQ = s dS^ K^                                  dK = s dS^T^ Q^

``rounding=False`` removes the five roundings: the formulas of tests/attn_grad_ref.py, written out by hand instead of by autograd.  ``defect`` plants what a
wrong kernel could do (``DEFECTS``).  ``keep``: per view ``None`` or a bool [nk] key mask on top of the table.

``tiled=True`` runs the forward as the kernel does, and in fp64 it is the yardstick of the rounded rule (tests/grad_parity.py ``compare_rounded``): what the
kernels compute when only their fp32 accumulation is taken away.  It is valid as that because it rounds p where ``attn_fwd_bf16`` does, read against
csrc/train_attn16.hip and csrc/train_attn.hpp:
  * tiles are the 64 keys [k0, k0 + 64) with k0 a multiple of 64 counted from key 0 of the VIEW (``ta_next_tile_m(v, 0, .)`` steps by TA_T from 0), not from
    the first valid key and not from the start of the key group: the loop below over ``range(0, nk, 64)``;
  * inside a tile p = exp(S - mn) with mn = max(running maximum, the tile's maximum over its valid keys) and is rounded as that value (``tb_pack`` on the
    accumulators that hold ``exp2f(s - ms)``); the running O and l are rescaled by exp(m - mn) in fp32 and never rounded;
  * l sums the p before the rounding (``sum += p`` ahead of ``tb_pack``);
  * a tile the kernel passes over -- wholly inside the skip range, at or past nk, or with no mask bit (``ta_tile_skipped_m``) -- contributes nothing, and so does
    a tile it does run although none of its keys is valid (the rule on tiles asks for the WHOLE tile inside the skip range, so nk = 70 with the skip [0, 70)
    runs the tile at 64; a skip range and a mask row can also empty a tile between them): there every s is -inf, mn = m, alpha = exp2(m - m) = 1 (or
    exp2(-inf - 0) = 0 on an accumulator that is still 0), every p is 0.  Both are the ``continue`` on a tile without a valid key below;
  * the backward has no running maximum: P = exp(S - lse) per element in all three kernels, rounded per element, so its tile order cannot be seen.
``exp2=True`` (fp32 and tiled only) is the kernel's own form of the exponentials, the host's stand-in for the GPU: ``TA_C`` = s log2 e as the fp32 constant
the header computes, applied in fp32 after the product, ``exp2``, O = acc * (1 / l), lse2 = m + log2 l, lse = lse2 * ``TA_LN2``, P = exp2(S c - lse2)."""
import torch

from attn_grad_ref import HEAD, make_case, valid_mask

S = 0.125
TA_C = float(torch.tensor(1.4426950408889634, dtype=torch.float32) * 0.125)          # train_attn.hpp: 0.125f * 1.4426950408889634f
TA_LN2 = float(torch.tensor(0.6931471805599453, dtype=torch.float32))
# what a wrong kernel could do: operands / P and dS truncated instead of rounded; l from the rounded p; delta from the rounded dO; s dropped on dK; P unrounded
# in dV; dP from the unrounded dO; dS unrounded as the operand of dQ only; V unrounded in the forward only
DEFECTS = ("truncate_operand", "truncate_p", "l_rounded", "delta_rounded", "dk_no_scale", "dv_unrounded_p", "dp_unrounded_do", "ds_unrounded_dq", "v_unrounded")


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


def core(case, dtype, rounding=True, defect=None, tiled=False, keep=None, exp2=False):
    """dict O, lse, dQ, dK, dV of a case of attn_grad_ref.make_case (q, k, v, dO, views, heads) in ``dtype``; lse [Rq, heads], -inf for a row without keys."""
    assert defect is None or defect in DEFECTS
    assert not exp2 or (tiled and dtype == torch.float32), "exp2 is the kernel's fp32 form"
    ex, lg, c = (torch.exp2, torch.log2, TA_C) if exp2 else (torch.exp, torch.log, S)
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
        v_fwd = _split(V, k0, nk, heads) if defect == "v_unrounded" else v
        s = (q @ k.transpose(1, 2)) * c          # in units of log 2 with exp2
        s = s.masked_fill(~valid, float("-inf"))
        if tiled:
            m = s.new_full((heads, nq, 1), float("-inf"))
            l, acc = s.new_zeros((heads, nq, 1)), s.new_zeros((heads, nq, HEAD))
            for t0 in range(0, nk, 64):
                st = s[:, :, t0:t0 + 64]
                if not bool(valid[t0:t0 + 64].any()):
                    continue
                mn = torch.maximum(m, st.max(-1, keepdim=True).values)
                alpha = ex(m - mn)
                p = ex(st - mn)
                l = l * alpha + (r_p(p) if defect == "l_rounded" else p).sum(-1, keepdim=True)
                acc = acc * alpha + r_p(p) @ v_fwd[:, t0:t0 + 64]
                m = mn
        else:
            m = s.max(-1, keepdim=True).values
            p = ex(s - m)
            l = (r_p(p) if defect == "l_rounded" else p).sum(-1, keepdim=True)
            acc = r_p(p) @ v_fwd
        o = acc * (1.0 / l) if exp2 else acc / l
        lse = m + lg(l)          # lse2 with exp2
        P = ex(s - lse)
        delta = ((r_op(do_raw) if defect == "delta_rounded" else do_raw) * o).sum(-1, keepdim=True)
        dv = (P if defect == "dv_unrounded_p" else r_p(P)).transpose(1, 2) @ do
        dS_raw = P * ((do_raw if defect == "dp_unrounded_do" else do) @ v.transpose(1, 2) - delta)
        dS = r_p(dS_raw)
        out["O"][q0:q0 + nq] = _merge(o)
        out["lse"][q0:q0 + nq] = (lse * TA_LN2 if exp2 else lse)[:, :, 0].t()
        out["dQ"][q0:q0 + nq] = _merge((dS_raw if defect == "ds_unrounded_dq" else dS) @ k) * S
        out["dK"][k0:k0 + nk] += _merge(dS.transpose(1, 2) @ q) * (1.0 if defect == "dk_no_scale" else S)
        out["dV"][k0:k0 + nk] += _merge(dv)
    return out


def written_rows(case, keep=None):
    """name -> bool [R]: the rows of O, dQ (queries) and of dK, dV (key range) that a view with queries and at least one valid key writes; every other row of
    the four tensors is an exact zero.  The segments ``grad_parity.compare_rounded`` counts."""
    rq, rk = torch.zeros(case["q"].shape[0], dtype=torch.bool), torch.zeros(case["k"].shape[0], dtype=torch.bool)
    for i, view in enumerate(case["views"]):
        q0, nq, k0, nk, _, _ = view
        valid = valid_mask(view)
        if keep is not None and keep[i] is not None:
            valid = valid & keep[i][:nk]
        if nq > 0 and nk > 0 and bool(valid.any()):
            rq[q0:q0 + nq] = True
            rk[k0:k0 + nk] = True
    return dict(O=rq, dQ=rq, dK=rk, dV=rk)


def key_mask_case():
    """(case, keep bool [views, 224]): cross_shared with the random key mask per view of test_masked_core_matches_the_reference_with_the_same_keys on top
    of its skips (seed 5, 0.6 kept, key 0 always, view 1 without a bit in the key tile [64, 128))."""
    case = make_case("cross_shared")
    keep = torch.rand((len(case["views"]), 224), generator=torch.Generator().manual_seed(5)) < 0.6
    keep[:, 0] = True
    keep[1, 64:128] = False
    return case, keep


def lse_rounded_bound(lse64, lse32):
    """(finite entries, bound): |lse - lse64| <= 4 max|lse32 - lse64| + 32 2^-24 max(1, max|lse64|) on every finite entry, no quantile: l sums the unrounded
    p, so no rounding flip reaches lse.  lse is a logarithm, of order 1 whatever the scores are, hence the floor of 1 on its magnitude."""
    fin = torch.isfinite(lse64)
    e_ref = float((lse32[fin].double() - lse64[fin]).abs().max())
    return fin, 4 * e_ref + 32 * 2.0 ** -24 * max(1.0, float(lse64[fin].abs().max()))


def lse_bound(q, k):
    """The single-key check of tests/test_attn16_gpu.py: (exact s sum q^ k^ in fp64, (64 + 8) 2^-24 s sum |q^| |k^|) for q [nq, 64] and one key k [64]:
    63 additions, the two constant multiplications and their constants' roundings, and headroom."""
    q64, k64 = rnd(q).double(), rnd(k).double()
    return S * (q64 * k64).sum(-1), (64 + 8) * 2.0 ** -24 * S * (q64.abs() * k64.abs()).sum(-1)

