"""Yardstick of memory dropout (must3r_amd/train_dropout.py, the masked kernels of csrc/train_attention.hip): tests/decoder_ref.call with key masks, in plain
torch, generic in dtype; the selection -- the (sel, not_sel) lists the reference's selectors return per call (blocks/dropout.py) -- is an input.  It composes
tests/decblock_ref.py (the block's other sublayers, prepare_y, memory_rows), tests/head_ref.py (the head) and tests/decoder_ref.py (the embedding, the feedback,
the tables, the case maker).  Also the fp64 formula of masked attention: the scores of dropped keys are set to -inf, and a row without a key gives zeros.
Nothing here imports must3r_amd.train_dropout."""
import torch

import block_ref as BR
import decblock_ref as DR
import decoder_ref as DF
import head_ref as HR
from must3r_amd import train_attention as TA
from oracle import must3r_ref as R

HEAD = 64
SCHEDULE = ((2, False), (3, False), (1, False), (2, False), (2, True))
P_DROP, PROTECTED_IMGS, SEED = 0.3, 1, 5


def make_case(mode="norm_y"):
    """B 2, n 35, Denc 128, D 64 / 1 head, depth 3, single_mlp, causal: an init of 2 views, 3 views over Nm = 70, a lone view, 2 views, a render of 2."""
    return DF.make_case(mode=mode, causal=True, schedule=SCHEDULE)


def valid_keys(view, keep=None):
    """bool [nk]: inside the table's range, outside its skip interval and, with ``keep`` (bool over at least a prefix of the keys), kept."""
    _, _, _, nk, lo, hi = view
    j = torch.arange(nk)
    ok = ~((j >= lo) & (j < hi))
    if keep is not None:
        k = torch.ones(nk, dtype=torch.bool)
        m = min(nk, keep.numel())
        k[:m] = keep[:m]
        ok = ok & k
    return ok


def attention(q, k, v, views, heads, keeps=None, lse_out=None):
    """O [Rq, heads * 64] in the dtype of q; ``keeps``: per view a bool tensor or None.  Scores of invalid keys are -inf; a row without a valid key gives 0
    (lse -inf).  lse_out: a dict that receives "lse" [Rq, heads] (natural log)."""
    o = q.new_zeros(q.shape)
    lse = q.new_full((q.shape[0], heads), float("-inf"))
    for i, view in enumerate(views):
        q0, nq, k0, nk, _, _ = view
        if nq == 0:
            continue
        valid = valid_keys(view, None if keeps is None else keeps[i]).to(q.device)
        if not bool(valid.any()):
            continue
        qh = q[q0:q0 + nq].reshape(nq, heads, HEAD).transpose(0, 1)
        kh = k[k0:k0 + nk].reshape(nk, heads, HEAD).transpose(0, 1)
        vh = v[k0:k0 + nk].reshape(nk, heads, HEAD).transpose(0, 1)
        s = (qh @ kh.transpose(1, 2) / 8).masked_fill(~valid, float("-inf"))
        o[q0:q0 + nq] = (torch.softmax(s, dim=-1) @ vh).transpose(0, 1).reshape(nq, heads * HEAD)
        lse[q0:q0 + nq] = torch.logsumexp(s.detach(), dim=-1).transpose(0, 1)
    if lse_out is not None:
        lse_out["lse"] = lse
    return o


def attention_grads(case, dtype):
    """dict O, lse, dQ, dK, dV of a case (q, k, v, dO, views, heads, keeps) under CPU autograd in ``dtype``"""
    q, k, v = (case[n].to(dtype).clone().requires_grad_(True) for n in ("q", "k", "v"))
    extra = {}
    o = attention(q, k, v, case["views"], case["heads"], case["keeps"], extra)
    o.backward(case["dO"].to(dtype))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(O=o.detach(), lse=extra["lse"], dQ=zero(q), dK=zero(k), dV=zero(v))


def cross_sublayer(x, mem, views, heads, p, kv_ready=False, eps=1e-6, keeps=None, keep=None):
    """decblock_ref.cross_sublayer with key masks"""
    D = heads * HEAD
    y = R.layer_norm(x, p["norm2.weight"], p["norm2.bias"], eps)
    q = y @ p["cross_attn.projq.weight"].t() + p["cross_attn.projq.bias"]
    if kv_ready:
        k, v = mem[:, :D], mem[:, D:]
    else:
        k = mem @ p["cross_attn.projk.weight"].t() + p["cross_attn.projk.bias"]
        v = mem @ p["cross_attn.projv.weight"].t() + p["cross_attn.projv.bias"]
        if keep is not None and k.requires_grad:
            k.retain_grad()
            keep["k"] = k
    o = attention(q, k, v, views, heads, keeps)
    return x + o @ p["cross_attn.proj.weight"].t() + p["cross_attn.proj.bias"]


def block(x, y, pos, self_views, mem_views, heads, p, mode, rope=(100.0, 1.0), eps=1e-6, keeps=None, keep=None):
    """decblock_ref.block with key masks in the cross attention"""
    x = BR.attention_sublayer(x, pos, self_views, heads, p, rope, eps)
    y_ = R.layer_norm(y, p["norm_y.weight"], p["norm_y.bias"], eps) if mode == "raw" else y
    x = cross_sublayer(x, y_, mem_views, heads, p, mode == "kv", eps, keeps, keep)
    return DR.mlp_sublayer(x, p, eps)


def sublayer_grads(case, dtype, which, keeps, extra=None):
    """decblock_ref.grads with key masks: which "cross" (a make_cross_case) or "block" (a make_block_case)"""
    x = case["x"].to(dtype).clone().requires_grad_(True)
    mem = case["mem"].to(dtype).clone().requires_grad_(True)
    p = {k: case["params"][k].to(dtype).clone().requires_grad_(True) for k in DR.param_names(case, which)}
    keep = {}
    if which == "cross":
        out = cross_sublayer(x, mem, case["views"], case["heads"], p, case["kv"], case["eps"], keeps, keep)
    else:
        y = DR.memory_rows(mem, DR.prepare_y(x, p, case["mode"], case["eps"]), case["scenes"])
        out = block(x, y, case["pos"], case["self_views"], case["views"], case["heads"], p, case["mode"], case["rope"], case["eps"], keeps, keep)
    out.backward(case["dy"].to(dtype))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = dict(out=out.detach(), dx=x.grad, dmem=zero(mem))
    res.update({k: zero(t) for k, t in p.items()})
    if extra is not None and "k" in keep:
        extra["dK_colsum"] = float(keep["k"].grad.abs().sum(dim=0).max())
    return res


def view_keeps(selection, B, V, Nk, render):
    """Per view of the call's table (scene-major) the keep mask of a selection (sel, not_sel), None where the reference masks nothing: an update hides
    not_sel[i] from view i in range(len(not_sel) - 1) (decoder.py:404); a render gathers the rows sel[0] for every view (decoder.py:478)."""
    if selection is None:
        return None
    sel, not_sel = selection
    rows = []
    for j in range(V):
        if render:
            keep = torch.zeros(Nk, dtype=torch.bool)
            keep[sel[0].long()] = True
            rows.append(keep)
        elif j < len(not_sel) - 1 and not_sel[j].numel():
            keep = torch.ones(Nk, dtype=torch.bool)
            keep[not_sel[j].long()] = False
            rows.append(keep)
        else:
            rows.append(None)
    return rows * B


def new_state():
    return dict(mem=None, n_imgs=0, prot_imgs=0, prot_tokens=0, labels=None)


def protected_tokens(state, V, n, render):
    """the `protected` argument of this call's draw (decoder.py:456-459)"""
    if render:
        return state["prot_tokens"]
    prot = min(PROTECTED_IMGS, state["prot_imgs"] + V)
    return state["prot_tokens"] + (prot - state["prot_imgs"]) * n


def call(case, p, x, state, render, selection, dropout_mode, keeps=None):
    """decoder_ref.call with the selection of the call: -> (state after the call, tokens [B V n, D] before norm_dec, pointmaps).  state: new_state()."""
    B, V, n, Denc = x.shape
    D, L, mode, eps, heads = case["D"], case["depth"], case["mode"], case["eps"], case["heads"]
    W = 2 * D if mode == "kv" else D
    mem = state["mem"]
    t = (x.reshape(-1, Denc) @ p["feat_embed_enc_to_dec.weight"].t() + p["feat_embed_enc_to_dec.bias"]).view(B, V, n, D)
    e = p["image2_embed"].view(1, 1, 1, D)
    t = torch.cat([t[:, :1], t[:, 1:] + e], dim=1) if mem is None else t + e
    xr = t.reshape(-1, D)
    Nm = 0 if mem is None else mem[0].shape[1]
    pos = case["pos"].repeat(B * V, 1)
    sv, cv = TA.self_views(B, V, n), DF.cross_table(B, V, n, Nm, render, True)
    Nk = Nm if render else Nm + V * n
    masked = render or Nm > 0 or V > 1
    if render and dropout_mode != "temporary":
        selection = None
    vk = view_keeps(selection, B, V, Nk, render) if masked else None
    new = []
    for l in range(L):
        bp = {k: p[f"blocks_dec.{l}.{k}"] for k in DR.PARAMS}
        if render:
            keys = mem[l].reshape(B * Nm, W)
        else:
            new.append(xr)
            py = DR.prepare_y(xr, bp, mode, eps)
            if mode == "kv":
                DF._watch(keeps, l, py)
            keys = py if Nm == 0 else DR.memory_rows(mem[l], py, B)
        keep = {}
        xr = block(xr, keys, pos, sv, cv, heads, bp, mode, case["rope"], eps, vk, keep)
        if "k" in keep and keeps is not None:
            keeps.append((l, keep["k"]))
    out = dict(state)
    if not render:
        if case["feedback_type"] and L > 1:
            off = DF.feedback_offset(new[-1], p, case["feedback_type"])
            new = [v + off for v in new[:-1]] + [new[-1]]
        rows = [DR.prepare_y(v, {k: p[f"blocks_dec.{l}.{k}"] for k in DR.PARAMS}, mode, eps).view(B, V * n, W) for l, v in enumerate(new)]
        if mode == "kv":
            for l, r in enumerate(rows):
                DF._watch(keeps, l, r)
        mem = rows if Nm == 0 else [torch.cat([m, r], dim=1) for m, r in zip(mem, rows)]
        labels = (torch.arange(V).view(1, V, 1).repeat(B, 1, n).view(B, V * n) + state["n_imgs"])
        labels = labels if state["labels"] is None else torch.cat([state["labels"], labels], dim=1)
        if selection is not None and dropout_mode == "permanent":
            mem, labels = [m[:, selection[0][-1].long()] for m in mem], labels[:, selection[0][-1].long()]
        prot = min(PROTECTED_IMGS, state["prot_imgs"] + V)
        out = dict(mem=mem, n_imgs=state["n_imgs"] + V, prot_imgs=prot, prot_tokens=state["prot_tokens"] + (prot - state["prot_imgs"]) * n, labels=labels)
    pts = HR.head(xr, p["norm_dec.weight"], p["norm_dec.bias"], p["head_dec.proj.weight"], p["head_dec.proj.bias"], B * V, case["H"], case["W"], eps)
    return out, xr, pts.view(B, V, case["H"], case["W"], HR.CHANNELS)


def grads(case, dtype, selections, dropout_mode, through="feats", extra=None):
    """decoder_ref.grads over the schedule with one selection per call: tokens{c}, feats{c}, pointmaps{c}, dx{c}, mem{l} of the final memory, one entry per
    parameter, "tail" (n_imgs, protected images, protected tokens) and "labels"."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in case["params"].items()}
    xs = [c["x"].to(dtype).clone().requires_grad_(True) for c in case["calls"]]
    keeps = [] if extra is not None else None
    state, loss, res = new_state(), 0, {}
    for i, (c, x, s) in enumerate(zip(case["calls"], xs, selections)):
        state, tok, pts = call(case, p, x, state, c["render"], s, dropout_mode, keeps)
        feats = R.layer_norm(tok, p["norm_dec.weight"], p["norm_dec.bias"], case["eps"])
        res[f"tokens{i}"], res[f"feats{i}"], res[f"pointmaps{i}"] = tok.detach(), feats.detach(), pts.detach()
        loss = loss + ((pts * c["G"].to(dtype)).sum() if through == "pointmaps" else (feats * c["T"].to(dtype)).sum())
    loss.backward()
    if extra is not None:
        D = case["D"]
        for l in range(case["depth"]):
            cols = sum(t.grad.reshape(-1, t.shape[-1])[:, :D].abs().sum(dim=0) for ll, t in keeps if ll == l and t.grad is not None)
            extra[f"blocks_dec.{l}.cross_attn.projk.bias"] = float(cols.max())
    res.update({f"mem{l}": m.detach() for l, m in enumerate(state["mem"])})
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    for k, t in p.items():
        if t.grad is not None:
            res[k] = t.grad
        elif not (through == "feats" and k.startswith("head_dec.")):
            res[k] = torch.zeros_like(t)
    res["tail"] = torch.tensor([state["n_imgs"], state["prot_imgs"], state["prot_tokens"]], dtype=torch.float64)
    res["labels"] = state["labels"]
    return res
