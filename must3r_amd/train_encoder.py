"""The encoder with a backward pass: the reference's ``Dust3rEncoder`` (must3r/model/encoder.py:13-52) -- dust3r's patch embedding, ``depth`` times ``Block``,
``norm_enc`` -- under ``torch.autograd``, and the training form of the reference's ``inference`` driver (must3r/engine/inference.py:595-688)::

    enc = Dust3rEncoder.from_encoder(native_encoder)                  # fp32 copies under the reference's state-dict keys
    x, pos = enc(img, true_shape)                                     # img [B, 3, H, W] fp32, true_shape [B, 2] -> x [B, N, E], pos int64 [B, N, 2]
    pts0, pts = inference(enc, dec, imgs, true_shape, [2, 1], encoder_requires_grad=True)      # dec: train_decoder.MUSt3R
    loss(pts0, pts).backward()                                        # enc.*.grad, dec.*.grad
    native_encoder.load_state_dict(enc.state_dict(), strict=True)     # serve what was trained

The patch embedding is a gather and a Linear: ``patch_rows`` (``must3r_hip_patch_rows``, include/must3r_hip.h "ABI 21, additive", csrc/train_encoder.hip) turns
the image batch into fp32 rows ``[B N, 768]`` in the column order of the flattened conv weight and writes the positions; ``train_block.linear_forward`` multiplies
the rows with ``proj.weight`` viewed as ``[E, 768]``.  ``ManyAR_PatchEmbed`` transposes the portrait views of a batch stored landscape: which views those are is
computed on the device (``true_shape[:, 0] > true_shape[:, 1]``) and read by the kernel, view by view; the host never learns it, nothing is split in two and one
encoder pass serves a batch of both orientations.  The backward gathers the rows again instead of keeping them (47 MB per 20 views of 384 x 512).

The blocks are ``train_block.Block`` on one view table and one ``pos`` tensor; ``norm_enc`` is ``train_block.layer_norm``.  The reference's encoder runs with
autocast disabled even under ``--amp bf16`` (encoder.py:46): ``precision="fp32"``, the default, enters the fp32 modes explicitly, so that an ambient
``train_block.amp("bf16")`` around encoder and decoder does what the reference's autocast does; ``"bf16"`` enters ``amp("bf16")``; ``None`` leaves the caller's
modes alone.  The forward reads nothing back to the host.  First order only; CPU tensors raise.

A decoder built with ``landscape_only=True`` (``train_decoder``) takes the mixed batch on: ``inference`` hands it the stored image size, so that the whole step from
the images to the pointmaps reads nothing back.

Not built: the image gradient (``img.requires_grad`` raises); ``forward_list``; DDP, activation
checkpointing and row chunking (a forward keeps two block inputs per layer: 3.0 GB at 24 layers, 20 views of 768 tokens); ``max_bs`` slicing under autograd.
"""
import contextlib
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import train_block as TB
from ._train_common import HEAD, _Affine, _dev, _f32, _record_modes, _recorded_modes, _rows, _stream
from .inference import _cumulative
from .model.blocks import parse_pos_embed
from .train_attention import _table, self_views
from .train_block import ROPE_NPOS
from .train_head import PredictionHead

PATCH = 16
PATCH_EMBEDS = ("PatchEmbedDust3R", "ManyAR_PatchEmbed")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the gather: the operator form, on a contiguous fp32 GPU tensor [V, 3, H, W]
# ---------------------------------------------------------------------------------------------------------------------------------------
def _check_img(img, what):
    """``(B, H, W)`` of an image batch; the shape is looked at before the device, so that a bad shape is reported as such wherever the tensor lives."""
    if not isinstance(img, torch.Tensor) or img.ndim != 4 or int(img.shape[1]) != 3 or img.numel() == 0:
        raise ValueError(f"{what}: img of shape {tuple(img.shape)}, expected [B, 3, H, W]")
    H, W = int(img.shape[2]), int(img.shape[3])
    if H % PATCH or W % PATCH:
        raise ValueError(f"{what}: an image of {H} x {W}, expected multiples of the patch size {PATCH}")
    return int(img.shape[0]), H, W


def patch_rows(img, transposed=None, want=(True, True)):
    """``must3r_hip_patch_rows``: img ``[V, 3, H, W]`` -> ``(rows fp32 [V N, 768], pos int64 [V N, 2])``, ``None`` where ``want`` says so; ``transposed``: int32
    ``[V]`` on the device, non-zero for a portrait view of a batch stored landscape (``None``: no view is)."""
    V, H, W = _check_img(img, "patch_rows")
    _dev(img, "patch_rows: img")
    if not any(want):
        return None, None
    img = _f32(img)
    dev, N = img.device, (H // PATCH) * (W // PATCH)
    if transposed is not None:
        _dev(transposed, "patch_rows: transposed")
        if transposed.dtype != torch.int32 or tuple(transposed.shape) != (V,):
            raise ValueError(f"patch_rows: transposed of dtype {transposed.dtype} and shape {tuple(transposed.shape)}, expected int32 [{V}]")
        transposed = transposed.contiguous()
    rows = torch.empty((V * N, 3 * PATCH * PATCH), dtype=torch.float32, device=dev) if want[0] else None
    pos = torch.empty((V * N, 2), dtype=torch.int64, device=dev) if want[1] else None
    a = _lib.PatchRowsArgs()
    a.img = img.data_ptr()
    a.transposed = None if transposed is None else transposed.data_ptr()
    a.rows = None if rows is None else rows.data_ptr()
    a.pos = None if pos is None else pos.data_ptr()
    a.V, a.H, a.W = V, H, W
    a.stream = _stream(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().must3r_hip_patch_rows(C.byref(a)))
    return rows, pos


# ---------------------------------------------------------------------------------------------------------------------------------------
# the patch embedding
# ---------------------------------------------------------------------------------------------------------------------------------------
def _embed_forward(img, weight, bias, flags):
    rows, pos = patch_rows(img, flags)
    E = int(weight.shape[0])
    x = TB.linear_forward(rows, _f32(weight).view(E, -1), _f32(bias))
    B = int(img.shape[0])
    return x.view(B, -1, E), pos.view(B, -1, 2)


class _PatchEmbed(torch.autograd.Function):
    """Saves the image, the weight and the flags; the backward gathers the rows again."""

    @staticmethod
    def forward(ctx, img, weight, bias, flags):
        ctx.save_for_backward(img, weight, bias, *([flags] if flags is not None else []))
        _record_modes(ctx, linear=True)
        x, pos = _embed_forward(img, weight, bias, flags)
        ctx.mark_non_differentiable(pos)
        return x, pos

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_x, _grad_pos):
        img, weight, bias, *flags = ctx.saved_tensors
        need = ctx.needs_input_grad
        E = int(weight.shape[0])
        rows, _ = patch_rows(img, flags[0] if flags else None, want=(True, False))
        with _recorded_modes(ctx):
            _, dW, db = TB.linear_grad(rows, _f32(weight).view(E, -1), _rows(grad_x), want=(False, bool(need[1]), bool(need[2])))
        return (None, None if dW is None else dW.view(weight.shape).to(weight.dtype), None if db is None else db.to(bias.dtype), None)


def patch_embed(img, weight, bias, true_shape=None, many_ar=False):
    """dust3r's ``PatchEmbedDust3R`` (``many_ar=False``: ``true_shape`` is ignored) or ``ManyAR_PatchEmbed``: img ``[B, 3, H, W]``, weight in the conv shape
    ``[E, 3, 16, 16]``, bias ``[E]``, true_shape ``[B, 2]`` (h, w) -> ``(x [B, N, E], pos int64 [B, N, 2])``.  Differentiable at weight and bias."""
    B, H, W = _check_img(img, "patch_embed")
    if weight.ndim != 4 or tuple(weight.shape[1:]) != (3, PATCH, PATCH) or tuple(bias.shape) != (int(weight.shape[0]),):
        raise ValueError(f"patch_embed: weight of shape {tuple(weight.shape)} and bias of shape {tuple(bias.shape)}, expected [E, 3, {PATCH}, {PATCH}] and [E]")
    if img.requires_grad:
        raise NotImplementedError("patch_embed: the gradient at the image is not built")
    flags = None
    if many_ar:
        if W < H:
            raise ValueError(f"patch_embed: ManyAR_PatchEmbed takes a batch stored landscape; this one is {H} x {W}")
        if true_shape is None or tuple(true_shape.shape) != (B, 2):
            raise ValueError(f"patch_embed: ManyAR_PatchEmbed needs true_shape [{B}, 2]")
    for t, name in ((img, "img"), (weight, "weight"), (bias, "bias")):
        _dev(t, f"patch_embed: {name}")
    if many_ar:
        ts = true_shape.to(img.device)
        flags = (ts[:, 0] > ts[:, 1]).to(torch.int32)      # on the device: nothing is read back
    if torch.is_grad_enabled() and (weight.requires_grad or bias.requires_grad):
        return _PatchEmbed.apply(img, weight, bias, flags)
    return _embed_forward(img, weight, bias, flags)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------------------
class _PatchEmbedParams(nn.Module):
    """``patch_embed.proj.weight`` / ``.bias`` in the conv shape, as dust3r's patch embeddings keep them (the Conv2d is a holder: it is never called)."""

    def __init__(self, kind, img_size, dim):
        super().__init__()
        self.kind, self.img_size, self.patch_size = kind, tuple(img_size), (PATCH, PATCH)
        self.grid_size = (self.img_size[0] // PATCH, self.img_size[1] // PATCH)
        self.proj = nn.Conv2d(3, dim, kernel_size=PATCH, stride=PATCH)


class Dust3rEncoder(nn.Module):
    """The reference's ``Dust3rEncoder`` as a trainable fp32 module; the parameters live under its state-dict keys (``patch_embed.proj.*``, ``blocks_enc.{i}.*``,
    ``norm_enc.*``), so that ``state_dict()`` loads into ``must3r_amd.model.Dust3rEncoder`` with ``strict=True``."""

    def __init__(self, img_size=(224, 224), patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, patch_embed="PatchEmbedDust3R",
                 pos_embed="RoPE100", precision="fp32", eps=1e-6, npos=ROPE_NPOS):
        super().__init__()
        if isinstance(img_size, int):
            img_size = (img_size, img_size)
        if int(patch_size) != PATCH:
            raise ValueError(f"Dust3rEncoder: patch_size {patch_size}, expected {PATCH}")
        if patch_embed not in PATCH_EMBEDS:
            raise ValueError(f"Dust3rEncoder: patch_embed {patch_embed!r}, expected one of {PATCH_EMBEDS}")
        if precision not in ("fp32", "bf16", None):
            raise ValueError(f"Dust3rEncoder: precision {precision!r}, expected 'fp32', 'bf16' or None")
        self.embed_dim, self.depth, self.patch_size, self.precision = int(embed_dim), int(depth), PATCH, precision
        self.eps, self.npos = float(eps), int(npos)
        self.patch_embed = _PatchEmbedParams(patch_embed, img_size, self.embed_dim)
        self.max_seq_len = max(img_size) // PATCH
        self.grid_size = self.patch_embed.grid_size
        self.rope = parse_pos_embed(pos_embed) if isinstance(pos_embed, str) else (float(pos_embed[0]), float(pos_embed[1]))   # a name, or (freq, F0)
        self.blocks_enc = nn.ModuleList([TB.Block(self.embed_dim, num_heads, mlp_ratio, self.rope, self.eps, self.npos) for _ in range(self.depth)])
        self.norm_enc = _Affine(self.embed_dim)

    @classmethod
    def from_encoder(cls, encoder, precision="fp32", **kw):
        """fp32 copies of a loaded ``must3r_amd.model.Dust3rEncoder`` (or anything with its state-dict keys and attributes); the source is left alone."""
        sd = encoder.state_dict()
        w = sd["patch_embed.proj.weight"]
        D = int(w.shape[0])
        depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks_enc."))
        hidden = int(sd["blocks_enc.0.mlp.fc1.weight"].shape[0])
        pe = encoder.patch_embed
        cfg = getattr(encoder, "cfg", None)
        enc = cls(img_size=tuple(getattr(pe, "img_size", (224, 224))), embed_dim=D, depth=depth,
                  num_heads=int(cfg.enc_heads) if cfg is not None else D // HEAD, mlp_ratio=hidden / D,
                  patch_embed=getattr(pe, "kind", type(pe).__name__), pos_embed=(cfg.rope_freq, cfg.rope_f0) if cfg is not None else "RoPE100",
                  precision=precision, eps=float(getattr(encoder.norm_enc, "eps", 1e-6)), **kw)
        enc.load_state_dict({k: v.detach().to(torch.float32).clone() for k, v in sd.items()}, strict=True)
        return enc.to(w.device)

    def from_dust3r(self, state_dict, verbose=True):   # encoder.py:54-61
        state_dict = {k.replace("enc_blocks", "blocks_enc").replace("enc_norm", "norm_enc"): v for k, v in state_dict.items()}
        inc = self.load_state_dict(state_dict, strict=False)
        if verbose:
            print(inc)
        assert len(inc.missing_keys) == 0
        return inc

    def from_croco(self, state_dict, verbose=True):
        return self.from_dust3r(state_dict, verbose=verbose)

    def forward(self, img, true_shape=None):
        """img ``[B, 3, H, W]`` fp32, true_shape ``[B, 2]`` (read by ``ManyAR_PatchEmbed`` alone) -> ``(x [B, N, E], pos int64 [B, N, 2])``."""
        B, H, W = _check_img(img, "Dust3rEncoder")
        if max(H, W) // PATCH > self.npos:
            raise ValueError(f"Dust3rEncoder: a grid of {max(H, W) // PATCH} positions a side, and a RoPE table of {self.npos}")
        pe = self.patch_embed
        with TB.amp(self.precision):
            x, pos = patch_embed(img, pe.proj.weight, pe.proj.bias, true_shape, pe.kind == "ManyAR_PatchEmbed")
            TB._positions_checked(pos, self.npos)      # in [0, max(H, W) / 16) by construction: the blocks do not read it on the host
            views = _table(self_views(1, B, int(x.shape[1])))
            for blk in self.blocks_enc:
                x = blk(x, pos, views)
            x = TB.layer_norm(x, self.norm_enc.weight, self.norm_enc.bias, self.eps)
        return x, pos


# ---------------------------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------------------------
def _grad_if(keep):
    """The caller's grad mode where ``keep``, ``no_grad`` otherwise."""
    return contextlib.nullcontext() if keep else torch.no_grad()


def inference(encoder, decoder, imgs, true_shape, mem_batches, train_decoder_skip=0, to_render=None, encoder_requires_grad=False, max_bs=None,
              verbose=False):
    """The reference's ``inference`` (engine/inference.py:595-688) under autograd: ``imgs`` ``[B, n, 3, H, W]``, ``true_shape`` ``[B, n, 2]`` (one aspect
    ratio; with a ``ManyAR_PatchEmbed`` encoder and a ``landscape_only=True`` decoder, rows of (W, H) for the portrait views of the batch stored landscape)
    -> ``(pointmaps_0 [B, sum(mem_batches) - skipped, H, W, C], pointmaps [B, n_rendered, H, W, C])``.  The encoder runs under ``no_grad`` unless
    ``encoder_requires_grad``, and so do the first ``train_decoder_skip`` memory updates, which do not contribute to ``pointmaps_0`` either; everything else
    stays in the graph.  Under ``torch.no_grad()`` this is ``must3r_amd.inference.inference``.  ``max_bs`` slicing is not built under autograd."""
    B, n = int(imgs.shape[0]), int(imgs.shape[1])
    if max_bs is not None and B * n > max_bs:
        raise NotImplementedError(f"train_encoder.inference: {B * n} images in slices of max_bs = {max_bs} are not built under autograd")
    with _grad_if(encoder_requires_grad):
        x, pos = encoder(imgs.reshape(B * n, *imgs.shape[2:]), true_shape.view(B * n, 2))
        x, pos = x.view(B, n, *x.shape[1:]), pos.view(B, n, *pos.shape[1:])
    # a landscape_only decoder learns the stored size from the image tensor: its head then reads nothing back from true_shape
    kw = dict(img_shape=(int(imgs.shape[-2]), int(imgs.shape[-1]))) if isinstance(decoder, PredictionHead) and decoder.landscape_only else {}
    bounds = _cumulative(mem_batches)
    mem, first_pass, out_shape = None, [], None
    for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        with _grad_if(b >= train_decoder_skip):
            mem, pm = decoder(x[:, lo:hi].contiguous(), pos[:, lo:hi].contiguous(), true_shape[:, lo:hi].contiguous(), mem, render=False, **kw)
        out_shape = out_shape or pm.shape
        if b >= train_decoder_skip:
            first_pass.append(pm)
    if first_pass:
        pointmaps_0 = torch.cat(first_pass, dim=1)
    else:
        pointmaps_0 = torch.empty((B, 0, *out_shape[2:]), dtype=x.dtype, device=x.device)
    if to_render is not None:
        x, pos, true_shape = x[:, to_render].contiguous(), pos[:, to_render].contiguous(), true_shape[:, to_render].contiguous()
        n = int(x.shape[1])
    assert mem is not None
    if verbose:
        print(f"Nmem={mem[0][-1].shape[1]}")
    if n == 0:
        return pointmaps_0, torch.empty((B, 0, *pointmaps_0.shape[2:]), dtype=x.dtype, device=x.device)
    _, pointmaps = decoder(x, pos, true_shape, mem, render=True, **kw)
    return pointmaps_0, pointmaps
