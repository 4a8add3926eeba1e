"""Offline reconstruction of a photo collection: ``must3r_inference`` of must3r/demo/inference.py:109-242 on the native path.

The reference reaches it from ``get_reconstruction.py --execution_mode retrieval|linseq`` and from demo/gradio.py:198-201.  Images
are read by ``must3r_amd.image.load_images``, encoded by ``inference.encoder_multi_ar``, ranked by ``retrieval.MUSt3R_Retriever``
(front-end + ASMK on the GPU), ordered by ``select_keyframes`` and reconstructed by ``inference.inference_multi_ar`` with
``engine.postprocess(compute_cam=True)``.  The video modes (``must3r_inference_video``) are not here.
"""
import datetime

import numpy as np
import torch

from .engine import postprocess
from .graph import farthest_point_sampling
from .image import load_images
from .inference import encoder_multi_ar, inference_multi_ar
from .model import get_dtype, get_pointmaps_activation
from .retrieval import MUSt3R_Retriever


class SceneState:
    """demo/inference.py:22-29"""

    def __init__(self, x_out, imgs, true_shape, focals, cams2world, image_list):
        self.x_out = x_out
        self.imgs = imgs
        self.true_shape = true_shape
        self.focals = focals
        self.cams2world = cams2world
        self.image_list = image_list


def rgb(img, true_shape=None):
    """dust3r.viz.rgb: a normalised [3, H, W] (or [H, W, 3]) image -> HWC float numpy, cropped to ``true_shape``, x * 0.5 + 0.5
    (uint8: / 255), clipped to [0, 1].  Lists are mapped element-wise."""
    if isinstance(img, list):
        return [rgb(x, true_shape=true_shape) for x in img]
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    if img.ndim == 3 and img.shape[0] == 3:
        img = img.transpose(1, 2, 0)
    elif img.ndim == 4 and img.shape[1] == 3:
        img = img.transpose(0, 2, 3, 1)
    if true_shape is not None:
        H, W = (int(v) for v in true_shape)
        img = img[:H, :W]
    img = np.float32(img) / 255 if img.dtype == np.uint8 else img * 0.5 + 0.5
    return img.clip(min=0, max=1)


def select_keyframes(sim_matrix, nimgs, num_mem_images, is_sequence):
    """demo/inference.py:138-173 -> the keyframe order (ints).  A sequence (or no scores): ``num_mem_images`` evenly spaced frames.
    Otherwise: ``num_mem_images`` farthest-point anchors of 1 - scores (one ``np.random.choice``), then a greedy chain over the
    anchors' scores with the diagonal cleared: start at the anchor of largest row sum, and repeatedly take the column of the
    largest score in the rows already taken, clearing each taken column."""
    if is_sequence or sim_matrix is None:
        return [int(i) for i in np.linspace(0, nimgs - 1, num_mem_images, dtype=int)]
    anchor_idx, _ = farthest_point_sampling(1 - sim_matrix, N=num_mem_images, dist_thresh=None)
    sim = sim_matrix[anchor_idx, :][:, anchor_idx]
    diag = np.diag_indices(num_mem_images)
    sim[diag[0], diag[1]] = 0
    chain = [np.argmax(np.sum(sim, axis=-1))]
    sim[:, chain[0]] = 0
    while len(chain) != num_mem_images:
        rows = sim[np.array(chain)]
        nxt = np.unravel_index(np.argmax(rows), rows.shape)[1]
        chain.append(nxt)
        sim[:, nxt] = 0
    return [int(anchor_idx[k]) for k in chain]


def memory_schedule(nimgs, num_mem_images, init_num_images, batch_num_views, render_once):
    """demo/inference.py:188-195, as the reference computes them -> (mem_batches, to_render)."""
    mem_batches = [min(init_num_images, nimgs)]
    while (sum_b := sum(mem_batches)) != max(num_mem_images, init_num_images):
        mem_batches.append(min(batch_num_views, num_mem_images - sum_b))
    to_render = list(range(num_mem_images, nimgs)) if render_once else None
    return mem_batches, to_render


def must3r_inference(model, retrieval, device, image_size, amp, filelist, num_mem_images, max_bs, init_num_images, batch_num_views,
                     render_once, is_sequence, viser_server=None, num_refinements_iterations=0, verbose=True):
    """demo/inference.py:109-242 -> ``SceneState``.  ``retrieval``: None, the retrieval checkpoint's path (as in the reference), or a
    ``MUSt3R_Retriever`` already built (a caller running many scenes loads the codebook once)."""
    dtype = get_dtype(amp)
    amp_on = dtype != torch.float32
    max_bs = None if max_bs == 0 else max_bs
    encoder, decoder = model
    pointmaps_activation = get_pointmaps_activation(decoder, verbose=verbose)

    def post_process_function(x):
        return postprocess(x, pointmaps_activation=pointmaps_activation, compute_cam=True)

    if verbose:
        print("loading images")
    time_start = datetime.datetime.now()
    views = load_images(filelist, size=image_size, patch_size=encoder.patch_size, verbose=verbose, device=device)
    if verbose:
        print(f"loaded in {datetime.datetime.now() - time_start}")
        print("running inference")
    time_start = datetime.datetime.now()
    if viser_server is not None:
        viser_server.reset(len(views))

    imgs = [b["img"] for b in views]
    true_shape = torch.stack([torch.from_numpy(b["true_shape"]) for b in views], dim=0)
    nimgs = true_shape.shape[0]

    encoder_precomputed_features = None
    if is_sequence or retrieval is None:
        keyframes = select_keyframes(None, nimgs, num_mem_images, True)
    else:
        with torch.autocast("cuda", dtype=dtype, enabled=amp_on):
            x_start, pos_start = encoder_multi_ar(encoder, imgs, true_shape, verbose=verbose, max_bs=max_bs, device=device,
                                                  preserve_gpu_mem=True)   # the tokens wait on the host, as in the reference (:144-145)
        encoder_precomputed_features = (x_start, pos_start)
        retriever = retrieval if isinstance(retrieval, MUSt3R_Retriever) else MUSt3R_Retriever(retrieval, backbone=encoder, verbose=verbose)
        sim_matrix = retriever([xi.unsqueeze(0).float() for xi in x_start], device=device)
        del retriever
        keyframes = select_keyframes(sim_matrix, nimgs, num_mem_images, False)

    not_keyframes = sorted(set(range(nimgs)).difference(set(keyframes)))
    assert len(keyframes) + len(not_keyframes) == nimgs
    order = keyframes + not_keyframes
    views = [views[i] for i in order]
    imgs = [b["img"].to(device) for b in views]
    true_shape = [torch.from_numpy(b["true_shape"]).to(device) for b in views]
    filenames = [filelist[i] for i in order]
    img_ids = [torch.tensor(v) for v in order]
    if encoder_precomputed_features is not None:
        x_start, pos_start = encoder_precomputed_features
        encoder_precomputed_features = ([x_start[i] for i in order], [pos_start[i] for i in order])

    mem_batches, to_render = memory_schedule(nimgs, num_mem_images, init_num_images, batch_num_views, render_once)
    with torch.autocast("cuda", dtype=dtype, enabled=amp_on):
        x_out_0, x_out = inference_multi_ar(encoder, decoder, imgs, img_ids, true_shape, mem_batches, max_bs=max_bs, verbose=verbose,
                                            to_render=to_render, encoder_precomputed_features=encoder_precomputed_features,
                                            device=device, preserve_gpu_mem=True, post_process_function=post_process_function,
                                            viser_server=viser_server, num_refinements_iterations=num_refinements_iterations)
    if to_render is not None:
        x_out = x_out_0 + x_out
    if verbose:
        print(f"inference in {datetime.datetime.now() - time_start}")
    if viser_server is not None:
        viser_server.reset_cam_visility()
        viser_server.send_message("Finished")

    focals = [float(x_out[i]["focal"].cpu()) for i in range(nimgs)]
    cams2world = [x_out[i]["c2w"].cpu() for i in range(nimgs)]
    for i in range(len(x_out)):
        for k in x_out[i].keys():
            x_out[i][k] = x_out[i][k].cpu()
    rgbimg = [rgb(imgs[i], true_shape[i]) for i in range(nimgs)]
    return SceneState(x_out, rgbimg, true_shape, focals, cams2world, filenames)
