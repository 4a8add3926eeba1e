"""``python -m must3r_amd.get_reconstruction``: images in a folder -> reconstruction -> ``scene_<thr>.glb`` / ``.ply`` for the eight
confidence thresholds + ``scene.pkl``, with the option names and defaults of the reference's get_reconstruction.py.

``load_model`` -> ``demo.get_reconstructed_scene(should_save_glb=False, ...)`` -> ``demo.export_scene_thresholds``: all eight files come
from one count + scan of the scene on the GPU and one scatter per threshold (must3r_amd.export).
"""
import argparse
import os
import pickle

from .demo import export_scene_thresholds, get_reconstructed_scene
from .export import REFERENCE_THRESHOLDS
from .model import MEMORY_MODES, load_model


def get_args_parser():
    p = argparse.ArgumentParser(prog="must3r_amd.get_reconstruction")
    p.add_argument("--image_size", type=int, default=512, choices=[512, 224], help="image size")
    p.add_argument("--image_dir", required=True, type=str, help="image dir")
    p.add_argument("--output", required=True, type=str, help="output dir")
    p.add_argument("--weights", type=str, default=None, help="path to the model weights")
    p.add_argument("--encoder", type=str, default=None, help="encoder class instantiation")
    p.add_argument("--decoder", type=str, default=None, help="decoder class instantiation")
    p.add_argument("--memory_mode", type=str, default=None, choices=MEMORY_MODES, help="decoder memory_mode override")
    p.add_argument("--retrieval", type=str, default=None, help="path to the retrieval weights")
    p.add_argument("--device", type=str, default="cuda", help="pytorch device")
    p.add_argument("--amp", type=str, default=False)
    p.add_argument("--execution_mode", type=str, default="linseq", choices=["linseq", "retrieval", "vidseq", "vidslam"])
    p.add_argument("--max_bs", type=int, default=1)
    p.add_argument("--num_refinements_iterations", type=int, default=0)
    p.add_argument("--render_once", action="store_true", default=False, help="skip the final rendering step")
    p.add_argument("--num_mem_imgs", type=int, default=50, help="linseq / retrieval: number of memory images")
    p.add_argument("--local_context_size", type=int, default=0, help="vidseq / vidslam")
    p.add_argument("--keyframe_interval", type=int, default=3, help="vidseq")
    p.add_argument("--subsample", type=int, default=2, help="vidslam")
    p.add_argument("--min_conf_keyframe", type=float, default=1.5, help="vidslam")
    p.add_argument("--keyframe_overlap_thr", type=float, default=0.05, help="vidslam")
    p.add_argument("--overlap_percentile", type=float, default=85, help="vidslam")
    p.add_argument("--cam_size", type=float, default=0.05)
    p.add_argument("--camera_conf_thr", type=float, default=0.0)
    p.add_argument("--file_type", type=str, default="glb", choices=["glb", "ply"])
    return p


def get_cli_parser():
    """``get_args_parser()`` -- the reference's arguments, kept equal to them -- plus this project's own switches"""
    p = get_args_parser()
    p.add_argument("--gpu_decode", action="store_true", default=False,
                   help="decode baseline JPEGs on the GPU (must3r_amd.jpeg); every other file, and the default, go through Pillow")
    p.add_argument("--render_dir", type=str, default=None,
                   help="write headless previews there (must3r_amd.render): one PNG frame per input view from that view's own camera")
    p.add_argument("--render_views", type=int, default=0, help="with --render_dir: this many orbit frames after the per-view frames")
    p.add_argument("--render_mesh", action="store_true", default=False,
                   help="with --render_dir: draw the triangles of the exported mesh instead of points (the reference viewer's default, as_pointcloud=False)")
    return p


def main(argv=None):
    args = get_cli_parser().parse_args(argv)
    if args.render_mesh and args.render_dir is None:
        raise SystemExit("--render_mesh needs --render_dir")
    images = sorted(os.path.join(args.image_dir, f) for f in os.listdir(args.image_dir) if os.path.isfile(os.path.join(args.image_dir, f)))
    os.makedirs(args.output, exist_ok=True)
    if args.execution_mode == "retrieval" and args.retrieval is None:
        raise SystemExit("--execution_mode retrieval needs --retrieval")
    model = load_model(args.weights, encoder=args.encoder, decoder=args.decoder, device=args.device, img_size=args.image_size,
                       memory_mode=args.memory_mode)
    thresholds = list(REFERENCE_THRESHOLDS)
    scene, _ = get_reconstructed_scene(
        outdir=args.output, viser_server=None, should_save_glb=False, model=model, retrieval=args.retrieval, device=args.device,
        verbose=True, image_size=args.image_size, amp=args.amp, filelist=images, min_conf_thr=thresholds[-1], as_pointcloud=True,
        transparent_cams=False, local_pointmaps=False, cam_size=args.cam_size, num_mem_images=min(args.num_mem_imgs, len(images)),
        max_bs=args.max_bs, render_once=args.render_once, camera_conf_thr=args.camera_conf_thr,
        num_refinements_iterations=args.num_refinements_iterations, execution_mode=args.execution_mode,
        vidseq_local_context_size=args.local_context_size, keyframe_interval=args.keyframe_interval,
        slam_local_context_size=args.local_context_size, subsample=args.subsample, min_conf_keyframe=args.min_conf_keyframe,
        keyframe_overlap_thr=args.keyframe_overlap_thr, overlap_percentile=args.overlap_percentile, gpu_decode=args.gpu_decode,
        render_dir=args.render_dir, render_views=args.render_views, render_mesh=args.render_mesh)
    # the reference passes cam_size alone to its export calls: camera_conf_thr stays at its default there
    paths = export_scene_thresholds(args.output, scene, thresholds, file_type=args.file_type, as_pointcloud=True, transparent_cams=False,
                                    cam_size=args.cam_size, verbose=True)
    with open(os.path.join(args.output, "scene.pkl"), "wb") as f:
        pickle.dump(scene, f)
    return paths


if __name__ == "__main__":
    main()
