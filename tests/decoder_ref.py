"""Yardstick of the trainable decoder (must3r_amd/train_decoder.py, csrc/train_decoder.hip): the reference's MUSt3R.forward and CausalMUSt3R.forward
(decoder.py:267-350, :435-553, feedback_mechanism.py:39-53) over flattened rows in plain torch, generic in dtype, for B scenes and a schedule of calls whose
memory carries the autograd graph from call to call.  It composes tests/decblock_ref.py (the block, prepare_y, memory_rows), tests/head_ref.py (the head) and
the oracle's layer_norm and GELU.  Runs under CPU autograd in fp64 (truth) and in fp32 (the reference's own precision).  Also the seeded case maker of
tests/test_decoder_grad_host.py and tests/test_decoder_grad_gpu.py, and the fp64 formula of the feedback add + norm_y operator."""
import torch

import block_ref as BR
import decblock_ref as DR
import head_ref as HR
from must3r_amd import train_attention as TA
from oracle import must3r_ref as R

HEAD = 64
FEEDBACK_EPS = 1e-5          # nn.LayerNorm's default (feedback_mechanism.py:14)
# (views, render) per call: init with 2 views (empty memory, masked), a lone view over the memory, 2 views over Nm = 3 n (masked), a render of 2 views over 5 n
SCHEDULE = ((2, False), (1, False), (2, False), (2, True))


def feedback_params(feedback_type):
    if feedback_type == "single_mlp":
        return ("feedback_layer.fc1.weight", "feedback_layer.fc1.bias", "feedback_layer.fc2.weight", "feedback_layer.fc2.bias", "feedback_norm.weight",
                "feedback_norm.bias")
    if feedback_type == "single_linear":
        return ("feedback_layer.weight", "feedback_layer.bias", "feedback_norm.weight", "feedback_norm.bias")
    return ()


def param_names(depth, feedback_type):
    """the reference's state-dict order"""
    return (("image2_embed", "feat_embed_enc_to_dec.weight", "feat_embed_enc_to_dec.bias") + tuple(f"blocks_dec.{i}.{k}" for i in range(depth) for k in DR.PARAMS)
            + feedback_params(feedback_type) + ("norm_dec.weight", "norm_dec.bias", "head_dec.proj.weight", "head_dec.proj.bias"))


def make_params(Denc, D, hidden, depth, feedback_type, g):
    """The scale of decblock_ref.make_params: weights of the scale a trained Linear has, norms around 1, biases around 0.1.  The feedback's last Linear is not
    zero (the reference zero-inits it: the offset would vanish and its parameters would see no gradient)."""
    rn = lambda *s: torch.randn(s, generator=g)
    p = {"image2_embed": 0.1 * rn(1, 1, D), "feat_embed_enc_to_dec.weight": rn(D, Denc) * Denc ** -0.5, "feat_embed_enc_to_dec.bias": 0.1 * rn(D)}
    for i in range(depth):
        p.update({f"blocks_dec.{i}.{k}": v for k, v in DR.make_params(D, hidden, g).items()})
    if feedback_type == "single_mlp":
        p.update({"feedback_layer.fc1.weight": rn(4 * D, D) * D ** -0.5, "feedback_layer.fc1.bias": 0.1 * rn(4 * D),
                  "feedback_layer.fc2.weight": rn(D, 4 * D) * (4 * D) ** -0.5, "feedback_layer.fc2.bias": 0.1 * rn(D)})
    elif feedback_type == "single_linear":
        p.update({"feedback_layer.weight": rn(D, D) * D ** -0.5, "feedback_layer.bias": 0.1 * rn(D)})
    if feedback_type:
        p.update({"feedback_norm.weight": 1 + 0.1 * rn(D), "feedback_norm.bias": 0.1 * rn(D)})
    p.update({"norm_dec.weight": 1 + 0.1 * rn(D), "norm_dec.bias": 0.1 * rn(D), "head_dec.proj.weight": rn(HR.OUT, D) * D ** -0.5,
              "head_dec.proj.bias": 0.1 * rn(HR.OUT)})
    assert tuple(p) == param_names(depth, feedback_type)
    return p


def make_case(Denc=128, D=64, heads=1, hidden=256, depth=3, feedback_type="single_mlp", mode="norm_y", causal=False, scenes=2, grid=(5, 7), seed=71,
              schedule=SCHEDULE):
    """`scenes` scenes, views of a grid[0] x grid[1] token grid; per call the encoder features x [B, V, n, Denc] and two upstream gradients of order 1e-7:
    G on the pointmaps [B, V, H, W, 7] and T on the tokens after norm_dec [B V n, D] (what the reference's classes return in fp64)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    p = make_params(Denc, D, hidden, depth, feedback_type, g)
    n, H, Wd = grid[0] * grid[1], 16 * grid[0], 16 * grid[1]
    calls = []
    for V, render in schedule:
        calls.append(dict(V=V, render=render, x=rn(scenes, V, n, Denc), G=rn(scenes, V, H, Wd, HR.CHANNELS) * 1e-7, T=rn(scenes * V * n, D) * 1e-7))
    pos = BR.grid_positions(n, grid[1])
    return dict(Denc=Denc, D=D, heads=heads, hidden=hidden, depth=depth, feedback_type=feedback_type or None, mode=mode, causal=causal, scenes=scenes, n=n,
                H=H, W=Wd, grid=tuple(grid), calls=calls, params=p, pos=pos, rope=(100.0, 1.0), eps=1e-6)


def feedback_offset(x, p, feedback_type):
    """feedback_layer(feedback_norm(x)): a Mlp without a residual, or a Linear (feedback_mechanism.py:11-23, :48)"""
    y = R.layer_norm(x, p["feedback_norm.weight"], p["feedback_norm.bias"], FEEDBACK_EPS)
    if feedback_type == "single_mlp":
        h = R.gelu(y @ p["feedback_layer.fc1.weight"].t() + p["feedback_layer.fc1.bias"])
        return h @ p["feedback_layer.fc2.weight"].t() + p["feedback_layer.fc2.bias"]
    return y @ p["feedback_layer.weight"].t() + p["feedback_layer.bias"]


def feedback_prepare(xs, offset, gammas, betas, add_layers, eps=1e-6):
    """[LN_l(x_l + (l < add_layers ? offset : 0))]; gammas None: the add alone"""
    out = []
    for l, x in enumerate(xs):
        v = x + offset if l < add_layers else x
        out.append(v if gammas is None else R.layer_norm(v, gammas[l], betas[l], eps))
    return out


def cross_table(B, V, n, Nm, render, causal):
    if render:
        return [[(b * V + j) * n, n, b * Nm, Nm, 0, 0] for b in range(B) for j in range(V)]
    if V == 1 and Nm == 0:
        return [[b * n, n, b * n, n, 0, 0] for b in range(B)]        # decoder.py:293: a lone first view attends its own tokens
    return TA.memory_views(B, V, n, Nm, mask=True, causal=causal)


def _watch(keeps, l, t):
    if keeps is not None and t.requires_grad:
        t.retain_grad()
        keeps.append((l, t))


def call(case, p, x, mem=None, render=False, keeps=None):
    """One forward: x [B, V, n, Denc], mem a list of depth tensors [B, Nm, W] or None -> (new memory list, tokens [B V n, D] before norm_dec, pointmaps).
    keeps: a list that receives (layer, tensor) for every tensor of projected keys (its first D columns), with its gradient retained."""
    B, V, n, Denc = x.shape
    D, L, mode, eps, heads = case["D"], case["depth"], case["mode"], case["eps"], case["heads"]
    W = 2 * D if mode == "kv" else D
    t = (x.reshape(-1, Denc) @ p["feat_embed_enc_to_dec.weight"].t() + p["feat_embed_enc_to_dec.bias"]).view(B, V, n, D)
    e = p["image2_embed"].view(1, 1, 1, D)
    t = torch.cat([t[:, :1], t[:, 1:] + e], dim=1) if mem is None else t + e
    xr = t.reshape(-1, D)
    Nm = 0 if mem is None else mem[0].shape[1]
    pos = case["pos"].repeat(B * V, 1)
    sv, cv = TA.self_views(B, V, n), cross_table(B, V, n, Nm, render, case["causal"])
    new = []
    for l in range(L):
        bp = {k: p[f"blocks_dec.{l}.{k}"] for k in DR.PARAMS}
        if render:
            keys = mem[l].reshape(B * Nm, W)
        else:
            new.append(xr)
            py = DR.prepare_y(xr, bp, mode, eps)
            if mode == "kv":
                _watch(keeps, l, py)
            keys = py if Nm == 0 else DR.memory_rows(mem[l], py, B)
        keep = {}
        xr = DR.block(xr, keys, pos, sv, cv, heads, bp, mode, case["rope"], eps, keep)
        if "k" in keep and keeps is not None:
            keeps.append((l, keep["k"]))
    out = mem
    if not render:
        if case["feedback_type"] and L > 1:
            off = feedback_offset(new[-1], p, case["feedback_type"])
            new = [v + off for v in new[:-1]] + [new[-1]]
        rows = [DR.prepare_y(v, {k: p[f"blocks_dec.{l}.{k}"] for k in DR.PARAMS}, mode, eps).view(B, V * n, W) for l, v in enumerate(new)]
        if mode == "kv":
            for l, r in enumerate(rows):
                _watch(keeps, l, r)
        out = rows if Nm == 0 else [torch.cat([m, r], dim=1) for m, r in zip(mem, rows)]
    pts = HR.head(xr, p["norm_dec.weight"], p["norm_dec.bias"], p["head_dec.proj.weight"], p["head_dec.proj.bias"], B * V, case["H"], case["W"], eps)
    return out, xr, pts.view(B, V, case["H"], case["W"], HR.CHANNELS)


def run(case, p, xs, keeps=None):
    """The schedule: [(tokens, pointmaps) per call], the final memory"""
    mem, outs = None, []
    for c, x in zip(case["calls"], xs):
        mem, tok, pts = call(case, p, x, mem, c["render"], keeps)
        outs.append((tok, pts))
    return outs, mem


def grads(case, dtype, through="pointmaps", extra=None):
    """dict under CPU autograd in ``dtype``: tokens{c} (before norm_dec), feats{c} (after), pointmaps{c}, dx{c} per call, mem{l} of the final memory and one
    entry per parameter.  The loss is sum_c <pointmaps_c, G_c> (``through="pointmaps"``) or sum_c <norm_dec(tokens_c), T_c> (``"feats"``: then the head's
    Linear has no gradient and no entry).  extra: a dict that receives, per layer, "blocks_dec.{l}.cross_attn.projk.bias" -> max_c sum_r |dK_rc| over every tensor
    of projected keys of the schedule: the magnitude of what cancels in that bias's gradient (every key a view sees carries the bias: the true gradient is 0)."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in case["params"].items()}
    xs = [c["x"].to(dtype).clone().requires_grad_(True) for c in case["calls"]]
    keeps = [] if extra is not None else None
    outs, mem = run(case, p, xs, keeps)
    loss, res = 0, {}
    for i, (c, (tok, pts)) in enumerate(zip(case["calls"], outs)):
        feats = R.layer_norm(tok, p["norm_dec.weight"], p["norm_dec.bias"], case["eps"])
        res[f"tokens{i}"], res[f"feats{i}"], res[f"pointmaps{i}"] = tok.detach(), feats.detach(), pts.detach()
        loss = loss + ((pts * c["G"].to(dtype)).sum() if through == "pointmaps" else (feats * c["T"].to(dtype)).sum())
    loss.backward()
    if extra is not None:
        D = case["D"]
        for l in range(case["depth"]):
            cols = sum(t.grad.reshape(-1, t.shape[-1])[:, :D].abs().sum(dim=0) for ll, t in keeps if ll == l and t.grad is not None)
            extra[f"blocks_dec.{l}.cross_attn.projk.bias"] = float(cols.max())
    res.update({f"mem{l}": m.detach() for l, m in enumerate(mem)})
    res.update({f"dx{i}": x.grad for i, x in enumerate(xs)})
    for k, t in p.items():
        if t.grad is not None:
            res[k] = t.grad
        elif not (through == "feats" and k.startswith("head_dec.")):
            res[k] = torch.zeros_like(t)
    return res
