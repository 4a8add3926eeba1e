"""A/B of the host side of the inference path (csrc/model.hip) between two builds of libmust3r_hip.so: same kernels, so every output must be bit-identical and every
profile row must count the same launches.

    python scripts/ab_model_stages.py --lib <libmust3r_hip.so> --out a.json      once per library, each in a fresh process (GPU)
    python scripts/ab_model_stages.py --diff a.json b.json                        on the host: exit status 1 on any difference

Per case the record holds the SHA-256 of every output tensor (encoder tokens and positions, pointmaps, all layers' memory rows [0, n_mem), feats) and the full profile
dictionaries of the encoder's and the decoder's context, ``k:`` symbol rows included.  The diff compares every hash and every row's call count (the times differ by
nature) and reports cases missing on either side; the LNFOLD256 case counts as not run unless the fold kernels (``k:g256sf/``, ``k:g256pf/``) show in its profile."""
import argparse
import dataclasses
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

H, W, MB = 48, 64, [2, 1, 1]


def sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def run_all(out_path):
    import torch
    from must3r_amd import _lib, synthetic as S
    from must3r_amd.config import ModelConfig, MUST3R_512
    from must3r_amd.engine import run_scenes, run_scenes_mixed
    from must3r_amd.parallel import ContextParallel
    import must3r_amd.model as M

    FOLD = ModelConfig(img_size=224, enc_dim=256, enc_depth=2, enc_heads=4, dec_dim=768, dec_depth=3, dec_heads=12)
    results = {}

    def modules(cfg, precision, mode="kv", feedback="single_mlp", cls=M.MUSt3R, **kw):
        enc = M.Dust3rEncoder(img_size=(cfg.img_size,) * 2, embed_dim=cfg.enc_dim, depth=cfg.enc_depth, num_heads=cfg.enc_heads, precision=precision)
        dec = cls(img_size=(cfg.img_size,) * 2, enc_embed_dim=cfg.enc_dim, embed_dim=cfg.dec_dim, depth=cfg.dec_depth, num_heads=cfg.dec_heads,
                  feedback_type=feedback, memory_mode=mode, landscape_only=False, precision=precision, **kw)
        enc.load_state_dict(S.make_encoder_state_dict(cfg, 0), strict=True)
        dec.load_state_dict(S.make_decoder_state_dict(cfg, 0, feedback_type=feedback), strict=True)
        return enc.cuda().eval(), dec.cuda().eval()

    def case(name, enc, dec, fn, options=()):
        ctxs = {"enc": enc._context(), "dec": dec._context()}
        try:
            for k, v in options:
                _lib.set_option(k, v)
            for c in ctxs.values():
                c.set_profiling(True)
                c.get_profile()
            tensors = fn()
            torch.cuda.synchronize()
            prof = {k: c.get_profile() for k, c in ctxs.items()}
        finally:
            for c in ctxs.values():
                c.set_profiling(False)
            for k, _ in options:
                _lib.set_option(k, {"LNFOLD": 1, "LNFOLD256": 0, "ENC_CHUNK_ROWS": 32768}[k])
        results[name] = {"sha256": {k: sha(t) for k, t in tensors.items()}, "profile": prof}
        print(name, len(tensors), "tensors", {k: sum(r["calls"] for n, r in p.items() if not n.startswith("k:")) for k, p in prof.items()}, flush=True)

    def mem_rows(out, mem):
        for l, v in enumerate(mem[0]):
            out[f"mem{l}"] = v

    def scene(enc, dec, V=4, mb=MB, feats=False, cp=None):
        """encode V views, update with the schedule, render all views: the calls of engine.run_scene one by one"""
        def fn():
            imgs, ts = S.make_images(V, H, W, 2)
            x, pos = enc(imgs.cuda(), ts)
            out, mem, i = {"x": x, "pos": pos}, None, 0
            for step, n in enumerate(mb):
                kw = {}
                if cp is not None and mem is not None and n == 1:
                    cp.n_mem_total = int(mem[0][0].shape[1])
                    kw["cp"] = cp
                r = dec(x[i:i + n].unsqueeze(0), pos[i:i + n].unsqueeze(0), ts[i:i + n].unsqueeze(0), mem, return_feats=feats, **kw)
                mem, out[f"update{step}"] = r[0], r[1]
                if feats:
                    out.update({f"update{step}_feats{l}": f for l, f in enumerate(r[2])})
                i += n
            r = dec(x.unsqueeze(0), pos.unsqueeze(0), ts.unsqueeze(0), mem, render=True, return_feats=feats)
            out["render"] = r[1]
            if feats:
                out.update({f"render_feats{l}": f for l, f in enumerate(r[2])})
            mem_rows(out, mem)
            return out
        return fn

    # the four precisions; the one-view fold off / on / with block 0's norm1 in the two split-weight modes
    for precision in ("bf16", "fp16", "fp16w2", "fp16wa"):
        enc, dec = modules(FOLD, precision)
        case(f"scene/{precision}", enc, dec, scene(enc, dec))
        if precision in ("fp16w2", "fp16wa"):
            for lnfold in (0, 2):
                case(f"scene/{precision}/LNFOLD={lnfold}", enc, dec, scene(enc, dec), options=[("LNFOLD", lnfold)])
    enc, dec = modules(FOLD, "fp16wa")
    case("scene/return_feats", enc, dec, scene(enc, dec, feats=True))
    for p16 in (True, False):
        case(f"scene/context_parallel/world1/partial16={int(p16)}", enc, dec, scene(enc, dec, cp=ContextParallel(None, partial16=p16)))
    # encoder alone: one view; three chunks with a shorter last one (44 views of 12 tokens at 256 rows per chunk: 15 + 15 + 14)
    def encode(n, seed):
        imgs, ts = S.make_images(n, H, W, seed)
        x, pos = enc(imgs.cuda(), ts)
        return {"x": x, "pos": pos}
    case("encoder/one_view", enc, dec, lambda: encode(1, 5))
    case("encoder/three_chunks", enc, dec, lambda: encode(44, 6), options=[("ENC_CHUNK_ROWS", 256)])
    for mode in ("norm_y", "raw"):
        e2, d2 = modules(FOLD, "fp16wa", mode=mode)
        case(f"scene/memory_mode={mode}", e2, d2, scene(e2, d2))
    for feedback in ("single_linear", None):
        e2, d2 = modules(FOLD, "fp16wa", feedback=feedback)
        case(f"scene/feedback={feedback}", e2, d2, scene(e2, d2))

    # the causal forward: three views in one call against an empty memory, then two more against it
    e2, d2 = modules(FOLD, "fp16wa", cls=M.CausalMUSt3R)

    def causal():
        imgs, ts = S.make_images(5, H, W, 3)
        x, pos = e2(imgs.cuda(), ts)
        mem, pm0 = d2(x[:3].unsqueeze(0), pos[:3].unsqueeze(0), ts[:3].unsqueeze(0), None)
        mem, pm1 = d2(x[3:].unsqueeze(0), pos[3:].unsqueeze(0), ts[3:].unsqueeze(0), mem)
        out = {"x": x, "update0": pm0, "update1": pm1}
        mem_rows(out, mem)
        return out
    case("causal", e2, d2, causal)

    # three scenes per call, update and render: one group with the update pointmaps written into slices of one buffer (pointmaps_scene_stride larger than a
    # scene: engine.run_scenes), two groups of different aspect ratio (forward_list calls: engine.run_scenes_mixed)
    def batched():
        imgs = torch.stack([S.make_images(4, H, W, 10 + b)[0] for b in range(3)]).cuda()
        r = run_scenes(enc, dec, imgs, S.make_images(4, H, W, 0)[1], mem_batches=MB, activate=False)
        out = {"x": r["x"], "update": r["update"], "render": r["render"]}
        mem_rows(out, r["mem"])
        return out
    case("batched/one_group", enc, dec, batched)

    def batched_mixed():
        groups = [torch.stack([S.make_images(n, h, w, 20 + b)[0] for b in range(3)]).cuda() for n, h, w in ((1, 48, 64), (2, 32, 64))]
        r = run_scenes_mixed(enc, dec, groups, mem_batches=[2, 1], activate=False)
        out = {f"update{i}": t for i, t in enumerate(r["update"])}
        out.update({f"render{i}": t for i, t in enumerate(r["render"])})
        mem_rows(out, r["mem"])
        return out
    case("batched/two_groups", enc, dec, batched_mixed)

    # LNFOLD256 = 1 on the launches that take it (tests/test_zz_r06_gpu.py test_model_fold256_switch_stays_inside_the_tolerance), both depths cut to 2
    cfg = dataclasses.replace(MUST3R_512, enc_depth=2, dec_depth=2)
    e3, d3 = modules(cfg, "fp16wa")

    def fold256():
        imgs, ts = S.make_images(20, 384, 512, 3)
        x, pos = e3(imgs.cuda(), ts)
        mem, upd = d3(x[:3].unsqueeze(0), pos[:3].unsqueeze(0), ts[:3].unsqueeze(0), None)
        x28, p28, t28 = torch.cat((x, x[:8])), torch.cat((pos, pos[:8])), torch.cat((ts, ts[:8]))
        _, ren = d3(x28.unsqueeze(0), p28.unsqueeze(0), t28.unsqueeze(0), mem, render=True)
        out = {"x": x, "pos": pos, "update": upd, "render": ren}
        mem_rows(out, mem)
        return out
    case("fold256", e3, d3, fold256, options=[("LNFOLD256", 1)])

    with open(out_path, "w") as f:
        json.dump({"cases": results}, f, indent=1, sort_keys=True)
    print("wrote", out_path, len(results), "cases")


def diff(a_path, b_path):
    a, b = (json.load(open(p))["cases"] for p in (a_path, b_path))
    bad = [f"case missing on one side: {n}" for n in sorted(set(a) ^ set(b))]
    hashes = rows = 0
    for name in sorted(set(a) & set(b)):
        ha, hb = a[name]["sha256"], b[name]["sha256"]
        for k in sorted(set(ha) | set(hb)):
            hashes += 1
            if ha.get(k) != hb.get(k):
                bad.append(f"{name}: tensor {k}: {ha.get(k)} != {hb.get(k)}")
        for ctx in ("enc", "dec"):
            pa, pb = a[name]["profile"][ctx], b[name]["profile"][ctx]
            for k in sorted(set(pa) | set(pb)):
                rows += 1
                ca, cb = (p.get(k, {}).get("calls") for p in (pa, pb))
                if ca != cb:
                    bad.append(f"{name}: {ctx} profile row {k}: {ca} != {cb} calls")
    for side, cases in (("a", a), ("b", b)):
        syms = [k for p in cases.get("fold256", {}).get("profile", {}).values() for k in p]
        if not (any(k.startswith("k:g256sf/") for k in syms) and any(k.startswith("k:g256pf/") for k in syms)):
            bad.append(f"fold256 ({side}): no k:g256sf/ and k:g256pf/ rows in the profile: the case counts as not run")
    print(f"{len(set(a) & set(b))} cases on both sides, {hashes} tensor hashes and {rows} profile rows compared, {len(bad)} differences")
    for line in bad:
        print("  " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--diff", nargs=2)
    args = ap.parse_args()
    if args.diff:
        sys.exit(diff(*args.diff))
    from must3r_amd import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)     # before the first load()
    run_all(args.out)
