"""Offline reconstruction of a photo collection or a video on the native path: must3r/demo/inference.py and the execution-mode
dispatch of demo/gradio.py:160-217 (``get_reconstruction.py --execution_mode linseq|retrieval|vidseq|vidslam``).

``must3r_inference`` (demo/inference.py:109-242): images are read by ``must3r_amd.image.load_images``, encoded by
``inference.encoder_multi_ar``, ranked by ``retrieval.MUSt3R_Retriever`` (front-end + ASMK on the GPU), ordered by
``select_keyframes`` and reconstructed by ``inference.inference_multi_ar`` with ``engine.postprocess(compute_cam=True)``.
``must3r_inference_video`` (:244-331): every frame in turn through ``inference.inference_video_multi_ar``; the keyframe test is a
callback, ``id % keyframe_interval == 0`` (vidseq) or ``slam_is_keyframe`` (vidslam: the overlap score of the frame against the
map of keyframe points, ``slam_nn.get_searcher("bvh-hip-quadrant_x2")``, which ``slam_update_scene_state`` grows).
``get_3D_model_from_scene`` / ``export_scene_thresholds`` (demo/gradio.py:75-156): GLB / PLY files from a ``SceneState`` through
``must3r_amd.export`` (compaction and transform on the GPU, no trimesh).
"""
import datetime
import functools

import numpy as np
import torch

from . import export as _export
from .engine import postprocess
from .graph import farthest_point_sampling
from .image import load_images
from .inference import encoder_multi_ar, inference_multi_ar, inference_video_multi_ar
from .model import get_dtype, get_pointmaps_activation
from .retrieval import MUSt3R_Retriever
from .slam_nn import choose_keyframe_from_overlap, get_overlap_score, get_searcher


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
                     render_once, is_sequence, viser_server=None, num_refinements_iterations=0, verbose=True, gpu_decode=False):
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
    views = load_images(filelist, size=image_size, patch_size=encoder.patch_size, verbose=verbose, device=device, decode="gpu" if gpu_decode else "pil")
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


def slam_is_keyframe(subsample, min_conf_keyframe, keyframe_overlap_thr, overlap_percentile, overlap_mode, id, res, scene_state):
    """demo/inference.py:79-93: a frame is a keyframe when its overlap score against the map is above the threshold ('nn' modes)."""
    cam_center = res["c2w"][:3, -1]
    res_unsqueeze = {k: v.unsqueeze(0).unsqueeze(0) for k, v in res.items()}
    overlap_score = get_overlap_score(res_unsqueeze, scene_state, cam_center=cam_center, mode=overlap_mode, kf_x_subsamp=subsample,
                                      min_conf_keyframe=min_conf_keyframe, percentile=overlap_percentile)
    assert not np.isnan(overlap_score)
    return choose_keyframe_from_overlap(overlap_score, keyframe_overlap_thr, overlap_mode)


def slam_update_scene_state(subsample, min_conf_keyframe, res, scene_state):
    """demo/inference.py:95-106: a keyframe's confident points (every ``subsample``-th row and column) join the map."""
    cam_center = res["c2w"][:3, -1]
    msk = res["conf"] > min_conf_keyframe
    if subsample:
        msk = msk[::subsample, ::subsample]
        pts = res["pts3d"][::subsample, ::subsample][msk]
    else:
        pts = res["pts3d"][msk]
    scene_state.add_pts(pts, cam_center=cam_center)
    return scene_state


def must3r_inference_video(model, device, image_size, amp, filelist, max_bs, init_num_images, batch_num_views, viser_server=None,
                           num_refinements_iterations=0, local_context_size: int = 25,
                           is_keyframe_function=lambda id, res, scene_state: (id % 3 == 0), scene_state=None,
                           scene_state_update_function=lambda res, scene_state: scene_state, verbose=True, gpu_decode=False):
    """demo/inference.py:244-331 -> ``SceneState``: the frames in file order, ``init_num_images`` of them first, then
    ``batch_num_views`` at a time, through ``inference_video_multi_ar`` with the keyframe and map callbacks."""
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
    views = load_images(filelist, size=image_size, patch_size=encoder.patch_size, verbose=verbose, device=device, decode="gpu" if gpu_decode else "pil")
    if verbose:
        print(f"loaded in {datetime.datetime.now() - time_start}")
        print("running inference")
    time_start = datetime.datetime.now()
    nimgs = len(views)
    if viser_server is not None:
        viser_server.reset(nimgs)

    imgs = [b["img"].to(device) for b in views]
    true_shape = [torch.from_numpy(b["true_shape"]).to(device) for b in views]
    filenames = filelist

    mem_batches = [min(init_num_images, nimgs)]
    while (sum_b := sum(mem_batches)) != nimgs:
        mem_batches.append(min(batch_num_views, nimgs - sum_b))

    with torch.autocast("cuda", dtype=dtype, enabled=amp_on):
        x_out = inference_video_multi_ar(encoder, decoder, imgs, true_shape, mem_batches, max_bs=max_bs, verbose=verbose, device=device,
                                         preserve_gpu_mem=True, post_process_function=post_process_function, viser_server=viser_server,
                                         num_refinements_iterations=num_refinements_iterations, local_context_size=local_context_size,
                                         is_keyframe_function=is_keyframe_function, scene_state=scene_state,
                                         scene_state_update_function=scene_state_update_function)
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


@torch.no_grad()
def get_reconstructed_scene(outdir, viser_server, should_save_glb, model, retrieval, device, verbose, image_size, amp,
                            filelist, max_bs, num_refinements_iterations,
                            execution_mode, num_mem_images, render_once, vidseq_local_context_size, keyframe_interval,
                            slam_local_context_size, subsample, min_conf_keyframe, keyframe_overlap_thr, overlap_percentile,
                            min_conf_thr, as_pointcloud, transparent_cams, local_pointmaps, cam_size, camera_conf_thr=0.0,
                            loaded_files="", gpu_decode=False, render_mesh=False, render_dir=None, render_views=0):
    """demo/gradio.py:160-217 -> ``(SceneState, None)``: the four execution modes with the reference's arguments.  The output
    parameters are accepted and unused, and ``should_save_glb=True`` is refused: export the returned scene with
    ``get_3D_model_from_scene`` or ``export_scene_thresholds``, as the reference's get_reconstruction.py does.  ``gpu_decode=True`` decodes the
    baseline JPEGs of the file list on the device (``load_images(..., decode="gpu")``, must3r_amd/jpeg.py); the default stays on Pillow.
    ``render_dir`` (default off) writes headless previews there (``render_previews``): one frame per input view from that view's own
    estimated camera, then ``render_views`` orbit frames; ``render_mesh=True`` draws them from the triangles of the exported mesh, not from points."""
    if should_save_glb:
        raise NotImplementedError("get_reconstructed_scene does not write the GLB / PLY file itself: call it with should_save_glb=False "
                                  "and pass the returned SceneState to get_3D_model_from_scene or export_scene_thresholds")
    if filelist:
        image_list = filelist
    elif loaded_files:
        image_list = loaded_files.split("\n")
    else:
        return None, None

    decode = dict(gpu_decode=True) if gpu_decode else {}   # without the switch the two drivers are called with the reference's arguments alone
    if execution_mode == "vidseq" or execution_mode == "vidslam":
        if execution_mode == "vidseq":
            local_context_size = vidseq_local_context_size

            def is_keyframe_function(id, res, scene_state):
                return id % keyframe_interval == 0
            scene_state = None

            def scene_state_update_function(res, scene_state):
                return scene_state
        else:
            local_context_size = slam_local_context_size
            overlap_mode = "nn-norm"
            is_keyframe_function = functools.partial(slam_is_keyframe, subsample, min_conf_keyframe, keyframe_overlap_thr,
                                                     overlap_percentile, overlap_mode)
            scene_state = get_searcher("bvh-hip-quadrant_x2")
            scene_state_update_function = functools.partial(slam_update_scene_state, subsample, min_conf_keyframe)
        scene = must3r_inference_video(model, device, image_size, amp, image_list, max_bs, init_num_images=2, batch_num_views=1,
                                       viser_server=viser_server, num_refinements_iterations=num_refinements_iterations,
                                       local_context_size=local_context_size, is_keyframe_function=is_keyframe_function,
                                       scene_state=scene_state, scene_state_update_function=scene_state_update_function,
                                       verbose=verbose, **decode)
    else:
        is_sequence = execution_mode == "linseq"
        scene = must3r_inference(model, retrieval, device, image_size, amp, image_list, num_mem_images, max_bs, init_num_images=2,
                                 batch_num_views=1, render_once=render_once, is_sequence=is_sequence, viser_server=viser_server,
                                 num_refinements_iterations=num_refinements_iterations, verbose=verbose, **decode)
    if render_dir is not None:
        render_previews(render_dir, scene, min_conf_thr, render_views, local_pointmaps=local_pointmaps, mesh=render_mesh)
    return scene, None


def render_previews(render_dir, scene, thr=3.0, n_orbit=0, local_pointmaps=False, point_size=2, mesh=False):
    """``frame_%05d.png`` in ``render_dir``: the cloud at confidence >= ``thr`` from every view's own camera (``render.view_camera``: the frame
    can be laid next to the input photo), then ``n_orbit`` frames from a circle around it, of the size of image 0 -> the list of paths.
    ``mesh=True``: the triangles of the exported mesh instead of squares of ``point_size`` pixels."""
    from . import render as _render
    cams = [_render.view_camera(scene, i) for i in range(len(scene.imgs))]
    if n_orbit > 0:
        H, W = (int(v) for v in scene.imgs[0].shape[:2])
        cams += _render.orbit_cameras(scene, n_orbit, thr, W, H, local_pointmaps=local_pointmaps)
    return _render.render_scene(render_dir, scene, cams, thr=thr, point_size=point_size, local_pointmaps=local_pointmaps, mesh=mesh)


@torch.no_grad()
def get_3D_model_from_scene(outdir, verbose, scene, min_conf_thr=3.0, as_pointcloud=False, transparent_cams=False, local_pointmaps=False,
                            cam_size=0.05, camera_conf_thr=0.0, filename="scene.glb"):
    """demo/gradio.py:131-156 -> the path of the written file (``None`` for ``scene is None``).  A file name ending in ``ply`` writes
    the point cloud alone (no cameras) and refuses mesh mode; anything else is a GLB with one wireframe frustum per camera whose median
    confidence reaches ``camera_conf_thr``.  ``transparent_cams`` is accepted and has no effect.  A threshold that selects nothing
    raises ``ValueError`` and writes no file."""
    if scene is None:
        return None
    path = _export.export_scene(outdir, scene, [min_conf_thr], [filename], as_pointcloud=as_pointcloud, transparent_cams=transparent_cams,
                                local_pointmaps=local_pointmaps, cam_size=cam_size, camera_conf_thr=camera_conf_thr, verbose=verbose)[0]
    if path is None:
        raise ValueError(f"get_3D_model_from_scene: no {'point' if as_pointcloud else 'triangle'} has confidence >= {min_conf_thr}")
    return path


@torch.no_grad()
def export_scene_thresholds(outdir, scene, thresholds, file_type="glb", **viz_args):
    """``scene_<thr>.<file_type>`` for every threshold (get_reconstruction.py:106-113) -> the list of written paths; a threshold that
    selects nothing is skipped.  One count + scan on the GPU serves up to 8 thresholds (more are chunked), one scatter each.
    ``viz_args``: ``as_pointcloud`` (default True, as the reference's CLI), ``transparent_cams``, ``local_pointmaps``, ``cam_size``,
    ``camera_conf_thr``, ``verbose``."""
    if scene is None:
        return []
    if file_type not in ("glb", "ply"):
        raise ValueError(f"export_scene_thresholds: file_type {file_type!r} is not 'glb' or 'ply'")
    viz_args.setdefault("as_pointcloud", True)
    names = [f"scene_{thr}.{file_type}" for thr in thresholds]
    return [p for p in _export.export_scene(outdir, scene, thresholds, names, **viz_args) if p is not None]
