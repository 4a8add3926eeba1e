"""GPU (-m gpu): must3r_amd/train.py -- ``train_one_epoch`` over ``train_data.SyntheticDepthScenes`` at the smallest geometry of the training tests: the D 64
decoder behind tests/golden/decoder_ref_d64.npz (Denc 128, D 64 / 1 head, hidden 256, depth 3, single_mlp) under an encoder of D 128 / depth 1, images of
32 x 48 (2 x 3 tokens), 4 views, B = 2, every third view portrait, ``train_dropout.CausalMUSt3R(landscape_only=True, mem_dropout=0.1)``.

The loop is held to the same four iterations written out by hand from the modules it binds: every parameter, both Adam moments, the step counts, the scaler
state and the returned averages bit for bit.  Under ``--amp bf16`` it is held to itself (bit-repeatable) and its averaged losses to the fp32 run's, within
the relative bound that profiles/attn16_parity.txt records for the decoder's output under amp (the row "decoder causal amp / tokens": bound = 4 e_ref + 32
in units of 2^-24 of the largest value; the head, the activation and the loss behind the tokens are fp32 in both runs and the loss is a mean of distances
between points, so a relative error of the points bounds the relative error of the loss)."""
import contextlib
import functools
import math
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import decoder_ref as DF
import encoder_ref as ER
from conftest import ROOT
from must3r_amd import train as T, train_block as TB, train_data as TDA, train_dropout as TDrop, train_encoder as TE, train_losses as TL, train_optim as TO
from must3r_amd.inference import concat_preds

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, NV, H, W = 2, 4, 32, 48
ITERS = 4


@functools.lru_cache(maxsize=None)
def _params():
    enc = ER.make_case(128, 2, 256, 1, B * NV, H, W, many_ar=True, seed=301)
    dec = DF.make_case(Denc=128, D=64, heads=1, hidden=256, depth=3, feedback_type="single_mlp", mode="norm_y", causal=True, scenes=B, grid=(H // 16, W // 16),
                       seed=302, schedule=())
    return enc, dec


def _modules(decoder_cls=TDrop.CausalMUSt3R):
    ec, dc = _params()
    enc = TE.Dust3rEncoder(img_size=(H, W), embed_dim=128, depth=1, num_heads=2, mlp_ratio=2.0, patch_embed="ManyAR_PatchEmbed")
    enc.load_state_dict(ec["params"], strict=True)
    dec = decoder_cls(landscape_only=True, mem_dropout=0.1, enc_embed_dim=128, embed_dim=64, depth=3, num_heads=1, mlp_ratio=4.0, feedback_type="single_mlp",
                      memory_mode="norm_y", rope=dc["rope"], eps=dc["eps"])
    inc = dec.load_state_dict(dc["params"], strict=False)
    assert not inc.unexpected_keys and set(inc.missing_keys) <= {"init_bias"}
    return enc.to(DEV), dec.to(DEV)


def _args(*argv, **kw):
    a = T.get_args_parser().parse_args(["--dataset", "SyntheticDepthScenes", "--epochs", "4", "--warmup_epochs", "2", "--lr", "1e-4", *argv])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _loader(n_batches=ITERS, seed=40, **kw):
    return DataLoader(TDA.SyntheticDepthScenes(B * n_batches, NV, H, W, seed=seed, portrait_every=3, **kw), batch_size=B)


def _setup(args, decoder_cls=TDrop.CausalMUSt3R):
    enc, dec = _modules(decoder_cls)
    groups = (TO.get_parameter_groups(enc, 0, args.weight_decay) if args.finetune_encoder else []) + TO.get_parameter_groups(dec, enc.depth, args.weight_decay)
    crit = eval(args.criterion, vars(TL) | {"args": args})
    return enc, dec, crit, TO.AdamW(groups, lr=args.lr, betas=(0.9, 0.95)), TO.LossScaler()


def _state(enc, dec, opt, scaler):
    """every parameter, the optimizer's moments and step counts, the scaler's state: clones"""
    out = {f"enc.{k}": v.detach().clone() for k, v in enc.named_parameters()}
    out.update({f"dec.{k}": v.detach().clone() for k, v in dec.named_parameters()})
    names = {id(p): n for n, p in [(f"enc.{k}", v) for k, v in enc.named_parameters()] + [(f"dec.{k}", v) for k, v in dec.named_parameters()]}
    for g in opt.param_groups:
        for p in g["params"]:
            for key, t in opt.state[p].items():
                out[f"{names[id(p)]}/{key}"] = t.detach().clone()
    torch.cuda.synchronize()
    return out, scaler.state_dict()


def _differ(a, b):
    assert set(a) == set(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


@contextlib.contextmanager
def _scalar_reads(log):
    """inside, every ``float(t)`` and ``t.item()`` appends ``t.is_cuda`` to ``log`` (``.tolist()``, the criterion's one read, is not among them)"""
    keep = torch.Tensor.__float__, torch.Tensor.item
    torch.Tensor.__float__ = lambda self: (log.append(self.is_cuda), keep[0](self))[1]
    torch.Tensor.item = lambda self: (log.append(self.is_cuda), keep[1](self))[1]
    try:
        yield
    finally:
        torch.Tensor.__float__, torch.Tensor.item = keep


@functools.lru_cache(maxsize=None)
def _loop_run(amp, repeat=0):
    """four iterations of train_one_epoch, accum_iter 2, the encoder fine-tuned: (state, scaler state, averages, initial parameters, scalar reads)"""
    args = _args("--finetune_encoder", "--accum_iter", "2", *(("--amp", amp) if amp else ()))
    enc, dec, crit, opt, scaler = _setup(args)
    before = {f"enc.{k}": v.detach().clone() for k, v in enc.named_parameters()}
    before.update({f"dec.{k}": v.detach().clone() for k, v in dec.named_parameters()})
    reads = []
    with _scalar_reads(reads):
        stats = T.train_one_epoch(enc, dec, crit, _loader(memory_num_views=3), opt, DEV, 1, scaler, args)
    state, sc = _state(enc, dec, opt, scaler)
    return state, sc, stats, before, reads


def _by_hand():
    """the same four iterations from the modules the loop binds"""
    args = _args("--finetune_encoder", "--accum_iter", "2")
    enc, dec, crit, opt, scaler = _setup(args)
    loader, epoch = _loader(memory_num_views=3), 1
    enc.train(True)
    dec.train(True)
    opt.zero_grad()
    torch.manual_seed(args.seed + epoch)
    np.random.seed(args.seed + epoch)
    rng = np.random.default_rng(seed=args.seed + epoch)
    sums = {}
    for it, batch in enumerate(loader):
        epoch_f = epoch + it / len(loader)
        if it % 2 == 0:
            TO.adjust_learning_rate(opt, epoch_f, args)
        imgs, ts, gt = TDA.collate_views(batch, DEV)
        imgs, ts, mnv, to_skip, to_render, skip_batches, mem_batches = T.select_batch(DEV, args, rng, int(batch[0]["memory_num_views"][0]), epoch_f / args.epochs,
                                                                                       imgs, ts, NV)
        assert (to_skip, to_render, skip_batches, mem_batches) == (0, None, [], [2, 1]) and mnv == 3
        with TB.amp("fp32"):
            p0, pts = TE.inference(enc, dec, imgs, ts, mem_batches, train_decoder_skip=0, to_render=None, encoder_requires_grad=True)
        pred = concat_preds(TL.postprocess(p0, "norm_exp"), TL.postprocess(pts, "norm_exp"))
        loss, details = crit(gt[:3] + gt, pred)
        value = float(loss.detach())
        assert math.isfinite(value)
        scaler(loss / 2, opt, parameters=None, update_grad=it % 2 == 1)
        if it % 2 == 1:
            opt.zero_grad()
        for k, v in dict(epoch=epoch_f, lr=opt.param_groups[0]["lr"], loss=value, **details).items():
            sums[k] = sums.get(k, 0.0) + v
    state, sc = _state(enc, dec, opt, scaler)
    return state, sc, {k: v / ITERS for k, v in sums.items()}


def test_four_iterations_are_the_hand_written_ones_bit_for_bit():
    state, sc, stats, before, reads = _loop_run(False)
    assert True not in reads, "train_one_epoch read a scalar from the device: the loss value comes from the criterion's details"
    ref_state, ref_sc, ref_stats = _by_hand()
    print(f"loop averages: {stats}")
    assert set(stats) == {"epoch", "lr", "loss", "conf_loss_g", "conf_loss_l", "Regr3D_pts3d", "Regr3D_pts3d_local"}
    assert stats == ref_stats, (stats, ref_stats)
    assert sc == ref_sc and sc["scale"] == 65536.0
    assert not _differ(state, ref_state)
    assert sum(k.endswith("/exp_avg") for k in state) == sum(k.endswith("/exp_avg_sq") for k in state) == len(before) and all(float(v) == 2.0 for k, v in state.items() if k.endswith("/step"))
    unchanged = [k for k, v in before.items() if torch.equal(v, state[k])]
    assert not unchanged, f"parameters the two updates left alone: {unchanged}"
    assert stats["lr"] == (1e-4 * 1.0 / 2 + 1e-4 * 1.0 / 2 + 1e-4 * 1.5 / 2 + 1e-4 * 1.5 / 2) / 4 and stats["epoch"] == (1 + 1.25 + 1.5 + 1.75) / 4


def _decoder_amp_bound():
    """profiles/attn16_parity.txt, row 'decoder causal amp / tokens': (4 e_ref + 32) 2^-24, relative to the largest value"""
    with open(os.path.join(ROOT, "profiles", "attn16_parity.txt")) as f:
        rows = [ln.split() for ln in f if ln.startswith("decoder causal amp") and " tokens: " in ln]
    assert len(rows) == 1
    m, e_gpu, e_ref, ratio = (float(x) for x in rows[0][-4:])
    assert abs(e_gpu / (4 * e_ref + 32) - ratio) < 1e-3          # the columns are the ones this reads them as
    return (4 * e_ref + 32) * 2.0 ** -24


def test_amp_bf16_runs_repeats_and_stays_within_the_recorded_bound_of_fp32():
    first, second, fp32 = _loop_run("bf16"), _loop_run("bf16", 1), _loop_run(False)
    assert first[2] == second[2] and first[1] == second[1] and not _differ(first[0], second[0])
    assert _differ(first[0], fp32[0]), "amp('bf16') changed nothing"
    bound = _decoder_amp_bound()
    for key in ("loss", "conf_loss_g", "conf_loss_l", "Regr3D_pts3d", "Regr3D_pts3d_local"):
        a, b = first[2][key], fp32[2][key]
        print(f"{key}: bf16 {a:.6f}, fp32 {b:.6f}, relative difference {abs(a - b) / abs(b):.3e} (bound {bound:.3e})")
    for key in ("loss", "conf_loss_g", "conf_loss_l", "Regr3D_pts3d", "Regr3D_pts3d_local"):
        a, b = first[2][key], fp32[2][key]
        assert math.isfinite(a) and abs(a - b) <= bound * abs(b), key


class _InitBias(TDrop.CausalMUSt3R):
    """a parameter that only the initialising update reaches"""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.init_bias = torch.nn.Parameter(torch.full((1, 1, 1, 128), 0.01))

    def forward(self, x, pos, true_shape, current_mem=None, render=False, **kw):
        if current_mem is None and not render:
            x = x + self.init_bias
        return super().forward(x, pos, true_shape, current_mem, render, **kw)


def test_skipped_updates_leave_no_graph():
    """memory_num_views 2 of 4 views, the last epoch of 4: the curriculum may skip two views, and does for the default seed (its first draw, checked here on
    the CPU).  One iteration of an accumulation of two: the gradients are still there afterwards."""
    grads = {}
    for name, mnv in (("skipped", "2"), ("whole", "10")):
        args = _args("--accum_iter", "2", "--memory_num_views", mnv)
        z = torch.zeros(B, NV, 1)
        _, _, _, to_skip, to_render, skip_batches, mem_batches = T.select_batch("cpu", args, np.random.default_rng(args.seed + 3), 2, 0.75, z, z, NV)
        assert (int(to_skip) > 0) == (name == "skipped") and (skip_batches, mem_batches) == (([2], [1]) if name == "skipped" else ([], [2]))
        enc, dec, crit, opt, scaler = _setup(args, _InitBias)
        stats = T.train_one_epoch(enc, dec, crit, _loader(1, memory_num_views=2), opt, DEV, 3, scaler, args)
        torch.cuda.synchronize()
        assert math.isfinite(stats["loss"])
        grads[name] = {k: v.grad for k, v in dec.named_parameters()}
        assert all(p.grad is None for p in enc.parameters())                 # not fine-tuned
        assert all(v is not None and bool(torch.isfinite(v).all()) for k, v in grads[name].items() if k != "init_bias")
    assert grads["skipped"]["init_bias"] is None
    assert grads["whole"]["init_bias"] is not None and float(grads["whole"]["init_bias"].abs().max()) > 0


class _Overflowing(TDrop.CausalMUSt3R):
    def forward(self, x, pos, true_shape, current_mem=None, render=False, **kw):
        mem, pm = super().forward(x, pos, true_shape, current_mem, render, **kw)
        if render:
            pm = pm.clone()
            pm[:, 0] = float("inf")
        return mem, pm


def test_a_non_finite_loss_ends_the_epoch_as_the_reference_does(capsys):
    args = _args("--accum_iter", "2")
    enc, dec, crit, opt, scaler = _setup(args, _Overflowing)
    before = {k: v.detach().clone() for k, v in dec.named_parameters()}
    with pytest.raises(SystemExit) as e:
        T.train_one_epoch(enc, dec, crit, _loader(2), opt, DEV, 0, scaler, args)
    assert e.value.code == 1 and "stopping training" in capsys.readouterr().out
    assert all(p.grad is None for p in dec.parameters()) and all(torch.equal(v, before[k]) for k, v in dec.named_parameters())
