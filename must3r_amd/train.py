"""The training loop of the reference's recipe (must3r/engine/train.py) on this back-end: what binds the trainable modules into an epoch::

    args = get_args_parser().parse_args(["--dataset", "...", "--amp", "bf16", "--finetune_encoder"])
    args.pointmaps_activation = get_pointmaps_activation(decoder)
    criterion = eval(args.criterion, vars(train_losses) | {"args": args})
    optimizer = train_optim.AdamW(get_parameter_groups(decoder, encoder.depth, args.weight_decay), lr=args.lr, betas=(0.9, 0.95))
    loss_scaler = train_optim.LossScaler()
    for epoch in range(args.start_epoch, args.epochs):
        stats = train_one_epoch(encoder, decoder, criterion, data_loader, optimizer, device, epoch, loss_scaler, args)
        train_optim.save_model(args, epoch, encoder, decoder, optimizer, loss_scaler, "last")
    save_final_model(args, args.epochs, encoder, decoder)

``get_args_parser`` has the reference's option names and defaults.  Three options do nothing here and are accepted for the recipe's command lines:
``--use_memory_efficient_attention`` (the attention core is one kernel family), ``--disable_cudnn_benchmark`` and ``--disable_tf32`` (there is no cuDNN and no
TF32 on this path: fp32 products are fp32).  The distributed options parse; anything other than one process raises.

``select_batch`` is train.py:132-216: the curriculum that decides how many views update the memory without a graph, which views are rendered and how the
views are grouped into memory updates, with the reference's ``rng.choice`` and ``torch.randperm`` calls in its order -- on ``device="cpu"`` it returns the
reference's values for the same seeds (tests/golden/select_batch_cases.json).

``train_one_epoch`` is train.py:385-510 on ``train_encoder.inference``, ``train_block.amp``, ``train_losses.postprocess`` and the criterion, and
``train_optim``'s scaler and optimizer.  Where it differs from the reference:

* ``--amp fp16`` raises ``NotImplementedError``: the training kernels have fp32 and bf16 modes only.
* ``--max_batch_size`` follows ``train_encoder.inference``: a batch that would need slicing raises there (``max_bs`` slicing is not built under autograd).
* ``to_render`` is brought to the host once, with ``.tolist()``; the reference iterates the device tensor ``select_batch`` returned, one read per element.
* The loss value of the finite check and of the log is taken from the criterion's ``details`` (``loss_value_from_details``): the criterion makes one
  device-to-host read for them and the loss is the fp32 sum of two of the figures it read, so the sum is redone on the host in fp32 -- the same bits as
  ``float(loss)``, and no second read.  A criterion this does not know falls back to ``float(loss)``.
* The logger is ``MetricLogger`` of this module: ``update(**values)``, ``meters[name].global_avg`` (croco's sum / count) and a progress line every
  ``print_freq`` iterations.  croco's printed line is not promised.
* ``log_writer`` is any object with ``add_scalar(tag, value, step)``.
* A batch goes through ``train_data.collate_views``: a loader in the reference's format (``pts3d``, ``valid_mask``) and one that hands over ``depthmap`` and
  ``camera_intrinsics`` both work; the latter gets its ground truth built on the device.
* ``args.pointmaps_activation`` defaults to ``get_pointmaps_activation(decoder)`` where ``train(args)`` has not set it.

Not built: ``train(args)`` itself (building a dataset, ``eval``-ing the model strings, the epoch loop around the checkpoints), DDP and tensorboard.
(Crop, resize and colour augmentation of raw frames in front of the loop: ``train_augment.augment_views`` / ``AugmentedScenes``.)
"""
import argparse
import math
import os
import sys
from itertools import chain
from pathlib import Path

import numpy as np
import torch

from . import losses as _L
from . import train_block as TB
from . import train_losses
from .inference import concat_preds
from .model import get_pointmaps_activation
from .train_data import collate_views
from .train_encoder import inference
from .train_optim import adjust_learning_rate

DEFAULT_CRITERION = "ConfLoss(Regr3D(L21, norm_mode='?avg_dis', sky_loss_value=2, loss_in_log=args.loss_in_log), alpha=0.2)"


def get_args_parser():
    """The reference's parser (train.py:34-113): the same option names, types and defaults."""
    parser = argparse.ArgumentParser("DUST3R training", add_help=False)
    add = parser.add_argument
    # model and criterion
    add("--encoder", default="Dust3rEncoder()", type=str, help="dust3r encoder init")
    add("--decoder", default="CausalMUSt3R()", help="decoder init")
    add("--memory_num_views", default=10, type=int, help="max number of views to use when updating the memory")
    add("--memory_batch_views", default=None, type=int, help="max number of views of one memory update")
    add("--min_memory_num_views", default=2, type=int, help="min number of views to use when updating the memory")
    add("--causal", action="store_true", default=False, help="update the memory in a single forward")
    add("--ignore_dataloader_memory_num_views", action="store_true", default=False)
    render = parser.add_mutually_exclusive_group()
    render.add_argument("--render_once", action="store_true", default=False)
    render.add_argument("--disable_render", action="store_true", default=False)
    add("--max_render_count", default=None, type=int)
    add("--finetune_encoder", default=False, action="store_true", help="Also finetune dust3r's encoder")
    add("--loss_in_log", action="store_true", default=False)
    add("--criterion", default=DEFAULT_CRITERION, type=str, help="loss")
    chkpt = parser.add_mutually_exclusive_group()
    chkpt.add_argument("--dust3r_chkpt", default=None, type=str, help="path to dust3r encoder weights")
    chkpt.add_argument("--croco_chkpt", default=None, type=str, help="path to croco decoder weights")
    chkpt.add_argument("--chkpt", default=None, type=str, help="optional path to decoder weights")
    # dataset
    add("--dataset", required=True, type=str, help="training set")
    # training
    add("--seed", default=777, type=int, help="Random seed")
    add("--batch_size", default=2, type=int, help="Batch size per GPU (effective batch size is batch_size * accum_iter * # gpus")
    add("--accum_iter", default=2, type=int, help="Accumulate gradient iterations")
    add("--max_batch_size", default=None, type=int, help="refused where the batch would need slicing (train_encoder.inference)")
    add("--epochs", default=20, type=int, help="Maximum number of epochs for the scheduler")
    add("--weight_decay", type=float, default=0.05, help="weight decay (default: 0.05)")
    add("--lr", type=float, default=None, metavar="LR", help="learning rate (absolute lr)")
    add("--blr", type=float, default=1.5e-4, metavar="LR", help="base learning rate: absolute_lr = base_lr * total_batch_size / 256")
    add("--min_lr", type=float, default=0., metavar="LR", help="lower lr bound for cyclic schedulers that hit 0")
    add("--warmup_epochs", type=int, default=6, metavar="N", help="epochs to warmup LR")
    add("--warmup_lr", type=float, default=0., help="lr at the start of warm-up")
    add("--amp", choices=[False, "bf16", "fp16"], default=False, help="bf16: train_block.amp('bf16'); fp16 is not built")
    add("--use_memory_efficient_attention", action="store_true", help="accepted, does nothing here")
    add("--disable_cudnn_benchmark", action="store_true", default=False, help="accepted, does nothing here")
    add("--disable_tf32", action="store_true", default=False, help="accepted, does nothing here")
    # others
    add("--num_workers", default=8, type=int)
    add("--world_size", default=1, type=int, help="number of distributed processes: 1 here")
    add("--local_rank", default=-1, type=int)
    add("--dist_on_itp", action="store_true")
    add("--nodist", action="store_true")
    add("--dist_url", default="env://", help="url used to set up distributed training")
    add("--keep_freq", default=5, type=int, help="frequence (number of epochs) to save checkpoint in checkpoint-%d.pth")
    add("--print_freq", default=20, type=int, help="frequence (number of iterations) to print infos while training")
    # output dir
    add("--output_dir", default="./output/", type=str, help="path where to save the output")
    return parser


def check_single_process(args):
    """DDP is not built: more than one process raises."""
    if int(getattr(args, "world_size", 1)) != 1 or getattr(args, "distributed", False) or getattr(args, "dist_on_itp", False) \
            or int(os.environ.get("WORLD_SIZE", "1")) != 1:
        raise NotImplementedError("must3r_amd.train: distributed training (DDP) is not built; run one process")


def select_batch(device, args, rng, memory_num_views, progress, imgs, true_shape, nimgs):
    """train.py:132-216 -> ``(imgs, true_shape, memory_num_views, to_skip, to_render, to_skip_batches, mem_batches)``.  ``rng``: a numpy ``Generator``;
    ``torch.randperm`` draws from torch's global generator of ``device``.  ``to_render`` is ``None`` (all views), a list, or an index tensor on ``device``."""
    to_skip, to_render = 0, None
    if args.memory_num_views < nimgs:
        # part of the memory is updated without a graph; the curriculum lets more and more views in as training progresses
        memory_num_views = 1
        max_views = min(math.ceil(args.memory_num_views + progress * (nimgs - args.memory_num_views)), nimgs)
        to_skip = rng.choice(max_views - args.min_memory_num_views + 1)      # how many views go in without a graph
        if to_skip < args.min_memory_num_views:                                # the initialisation is not split
            to_skip, memory_num_views = 0, args.min_memory_num_views
        seen = to_skip + memory_num_views
        max_n_imgs = min(seen + args.memory_num_views, max_views)
        imgs, true_shape = imgs[:, :max_n_imgs].contiguous(), true_shape[:, :max_n_imgs].contiguous()
        number_unseen = max_n_imgs - seen
        if args.render_once:                                                   # the unseen views only
            to_render = torch.randperm(number_unseen, device=device) + seen if number_unseen > 0 else []
        else:                                                                  # half unseen views, half random seen ones
            to_render = (torch.randperm(number_unseen, device=device) + seen)[:math.ceil(args.memory_num_views / 2)]
            n_selected = len(to_render)
            to_render = torch.concatenate([to_render, torch.randperm(seen, device=device)[:(args.memory_num_views - n_selected)]])
    elif args.render_once:
        to_render = list(range(memory_num_views, nimgs))

    def split(total, draw):
        """sizes that add up to ``total``, each the next ``draw`` capped by what is left"""
        sizes = []
        while (done := sum(sizes)) != total:
            sizes.append(min(draw(total), total - done))
        return sizes

    to_skip_batches, mem_batches = [], []
    if to_skip > 0:
        assert to_skip >= args.min_memory_num_views
    if args.memory_batch_views is not None:
        if not args.causal:      # several views at once, a random number each time
            draw = lambda total: rng.choice(min(args.memory_batch_views, total)) + 1
        else:                    # several views at once, memory_batch_views at most
            draw = lambda total: args.memory_batch_views
        if to_skip > 0:
            to_skip_batches = split(to_skip, draw)
        mem_batches = split(memory_num_views, draw)
    elif not args.causal:        # dust3r-like: one view at a time after the initialisation
        if to_skip > 0:
            to_skip_batches = [args.min_memory_num_views] + [1] * (to_skip - args.min_memory_num_views)
            mem_batches = [1] * memory_num_views
        else:
            mem_batches = [args.min_memory_num_views] + [1] * (memory_num_views - args.min_memory_num_views)
    elif to_skip > 0:
        to_skip_batches = [to_skip]
    else:
        mem_batches = [memory_num_views]
    return imgs, true_shape, memory_num_views, to_skip, to_render, to_skip_batches, mem_batches


class Meter:
    """croco's ``SmoothedValue`` as far as the epoch's statistics use it: the last value, and ``global_avg`` = sum / count."""

    def __init__(self):
        self.total, self.count, self.value = 0.0, 0, float("nan")

    def update(self, value, n=1):
        self.value = value
        self.count += n
        self.total += value * n

    @property
    def global_avg(self):
        return self.total / self.count


class MetricLogger:
    """``update(name=value, ...)`` (numbers, or one-element tensors: read with ``.item()``), ``meters[name].global_avg``, and ``log_every`` around an iterable."""

    def __init__(self, delimiter="  "):
        self.meters, self.delimiter = {}, delimiter

    def update(self, **kwargs):
        for k, v in kwargs.items():
            if v is None:
                continue
            if isinstance(v, torch.Tensor):
                v = v.item()
            assert isinstance(v, (float, int)), (k, type(v))
            self.meters.setdefault(k, Meter()).update(v)

    def __str__(self):
        return self.delimiter.join(f"{k}: {m.global_avg:.4f}" for k, m in self.meters.items())

    def log_every(self, iterable, print_freq, header=""):
        n = len(iterable) if hasattr(iterable, "__len__") else None
        for i, obj in enumerate(iterable):
            yield obj
            if print_freq and (i % print_freq == 0 or (n is not None and i == n - 1)):
                last = self.delimiter.join(f"{k}: {m.value:.6g} ({m.global_avg:.6g})" for k, m in self.meters.items())
                print(self.delimiter.join(s for s in (header, f"[{i}/{n}]" if n is not None else f"[{i}]", last) if s))


def loss_value_from_details(criterion, loss, details):
    """The value of ``loss`` on the host without reading it: ``ConfLoss`` returns ``figures[2] + figures[3]`` in fp32 and the two figures, read once, as
    ``conf_loss_g`` and ``conf_loss_l`` of its details; the fp32 sum of the two is redone here (``float(loss)`` bit for bit).  Any other criterion, a scaled
    one or a sum of two: ``float(loss)``."""
    if isinstance(criterion, _L.ConfLoss) and criterion._alpha == 1 and criterion._loss2 is None and "conf_loss_g" in details:
        value = np.float32(details["conf_loss_g"])
        if "conf_loss_l" in details:
            with np.errstate(all="ignore"):
                value = value + np.float32(details["conf_loss_l"])
        return float(value)
    return float(loss)


def train_one_epoch(encoder, decoder, criterion, data_loader, optimizer, device, epoch, loss_scaler, args, log_writer=None):
    """train.py:385-510: one pass over ``data_loader`` -> the epoch's averages ``{name: global_avg}`` (``epoch``, ``lr``, ``loss`` and the criterion's details).
    ``encoder``: ``train_encoder.Dust3rEncoder``; ``decoder``: a ``train_decoder`` / ``train_dropout`` decoder; ``criterion``: ``train_losses``;
    ``optimizer`` / ``loss_scaler``: ``train_optim.AdamW`` / ``LossScaler``.  A non-finite loss ends the process with ``sys.exit(1)``, as the reference
    does.  The differences from the reference are listed in the module's docstring."""
    check_single_process(args)
    if args.amp == "fp16":
        raise NotImplementedError("must3r_amd.train: --amp fp16 is not built (the training kernels have fp32 and bf16 modes)")
    if args.amp not in (False, None, "bf16"):
        raise ValueError(f"must3r_amd.train: amp {args.amp!r}, expected False or 'bf16'")
    encoder.train(args.finetune_encoder)
    decoder.train(True)
    metric_logger = MetricLogger(delimiter="  ")
    header = "Epoch: [{}]".format(epoch)
    accum_iter = args.accum_iter
    if log_writer is not None and hasattr(log_writer, "log_dir"):
        print("log_dir: {}".format(log_writer.log_dir))
    for part in ("dataset", "sampler"):
        if hasattr(data_loader, part) and hasattr(getattr(data_loader, part), "set_epoch"):
            getattr(data_loader, part).set_epoch(epoch)
    optimizer.zero_grad()

    # fix the seed (one process: world size 1, rank 0)
    seed = args.seed + epoch
    torch.manual_seed(seed)
    np.random.seed(seed)
    rng = np.random.default_rng(seed=args.seed + epoch)

    activation = getattr(args, "pointmaps_activation", None)
    if activation is None:
        activation = get_pointmaps_activation(decoder, verbose=False)
    precision = "bf16" if args.amp == "bf16" else "fp32"
    for data_iter_step, batch in enumerate(metric_logger.log_every(data_loader, args.print_freq, header)):
        epoch_f = epoch + data_iter_step / len(data_loader)
        progress = epoch_f / args.epochs
        # a per iteration (instead of per epoch) lr scheduler
        if data_iter_step % accum_iter == 0:
            adjust_learning_rate(optimizer, epoch_f, args)

        imgs, true_shape, gt_views = collate_views(batch, device)      # B, nimgs, 3, H, W
        nimgs = int(imgs.shape[1])
        if args.ignore_dataloader_memory_num_views:
            memory_num_views = rng.choice(args.memory_num_views - args.min_memory_num_views + 1) + args.min_memory_num_views
        else:
            memory_num_views = int(batch[0]["memory_num_views"][0])
        imgs, true_shape, memory_num_views, to_skip, to_render, to_skip_batches, mem_batches = select_batch(
            device, args, rng, memory_num_views, progress, imgs, true_shape, nimgs)
        mem_batches = to_skip_batches + mem_batches
        if isinstance(to_render, torch.Tensor):
            to_render = to_render.tolist()                             # one read, not one per element
        if args.max_render_count is not None:
            if to_render is None:
                to_render = list(range(nimgs))
            to_render = rng.choice(to_render, size=args.max_render_count, replace=False).tolist()
        if args.disable_render:
            to_render = []
        with TB.amp(precision):
            x_out_0, x_out = inference(encoder, decoder, imgs, true_shape, mem_batches, train_decoder_skip=len(to_skip_batches),
                                       max_bs=args.max_batch_size, to_render=to_render, encoder_requires_grad=args.finetune_encoder)
        x_out_0 = train_losses.postprocess(x_out_0, pointmaps_activation=activation)
        x_out = train_losses.postprocess(x_out, pointmaps_activation=activation)
        b0 = list(gt_views[to_skip:(to_skip + memory_num_views)])
        br = list(gt_views) if to_render is None else [gt_views[i] for i in to_render]
        x_out = concat_preds(x_out_0, x_out)
        loss, loss_details = criterion(b0 + br, x_out)
        loss_value = loss_value_from_details(criterion, loss, loss_details)
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            sys.exit(1)

        loss = loss / accum_iter
        update_grad = (data_iter_step + 1) % accum_iter == 0
        parameters = chain(encoder.parameters(), decoder.parameters()) if args.finetune_encoder else decoder.parameters()
        loss_scaler(loss, optimizer, parameters=parameters, update_grad=update_grad)
        if update_grad:
            optimizer.zero_grad()
        del loss, batch, gt_views, x_out, x_out_0

        lr = optimizer.param_groups[0]["lr"]
        metric_logger.update(epoch=epoch_f)
        metric_logger.update(lr=lr)
        metric_logger.update(loss=loss_value, **loss_details)
        if update_grad and (data_iter_step + 1) % (accum_iter * args.print_freq) == 0 and log_writer is not None:
            epoch_1000x = int(epoch_f * 1000)      # the x-axis: calibrates curves of different batch sizes
            log_writer.add_scalar("train_loss", loss_value, epoch_1000x)
            log_writer.add_scalar("train_lr", lr, epoch_1000x)
            log_writer.add_scalar("train_iter", epoch_1000x, epoch_1000x)
            for name, val in loss_details.items():
                log_writer.add_scalar("train_" + name, val, epoch_1000x)
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def save_final_model(args, epoch, encoder, decoder):
    """train.py:371-382: ``args.output_dir/checkpoint-final.pth`` with the keys args, encoder, decoder, epoch (state dicts, or dicts given as such)."""
    checkpoint_path = Path(args.output_dir) / "checkpoint-final.pth"
    to_save = {"args": args, "encoder": encoder if isinstance(encoder, dict) else encoder.state_dict(),
               "decoder": decoder if isinstance(decoder, dict) else decoder.state_dict(), "epoch": epoch}
    print(f">> Saving model to {checkpoint_path} ...")
    torch.save(to_save, checkpoint_path)
    return checkpoint_path
