"""Launch trace of every denoising loop, recorded on the CPU (no GPU, no kernel runs).

    python tools/launch_trace.py [ROOT] [--dump DIR] [--only NAME ...]

Every kernel launch of the package goes through `ops._call(name, *args)`; with graphs off nothing else on the host side
of the loops touches the device.  This tool replaces `ops._call` by a recorder and `ops._stream` by a null pointer,
builds tiny engines on device "cpu" with use_graphs=False and runs each loop for a few steps through its public entry
point.  Per scenario it prints the number of recorded lines and a hash of their text; `--dump DIR` writes the text
itself (one file per scenario), so that two checkouts can be compared with `diff -r`:

    python tools/launch_trace.py /path/to/checkout_a --dump /tmp/a
    python tools/launch_trace.py /path/to/checkout_b --dump /tmp/b && diff -r /tmp/a /tmp/b

ROOT is the checkout to trace (the directory that holds lgd_amd.py), by default the one this file lies in.

A line is `name(arg, arg, ...)`: pointers are renamed by order of first appearance within the scenario, the fields of
an LgdGemmDesc are expanded, `ops.copy_` / `ops.zero_` (which bypass `_call`) are recorded as lines of their own, and
the step entry points carry a hash of the CONTENTS of their coefficient table (the host writes it, so it is real here).
Every tensor handed to `ops._p`, `ops.gemm_desc`, `ops.copy_` or `ops.zero_` is kept alive for the whole run: otherwise
the allocator reuses addresses and the renaming differs from run to run.

The `clip`, `owlvit` and `sam` scenarios trace the towers outside the UNet: tiny configs (tests/owl_detect_cases.py,
tests/sam_cases.py of the traced checkout) with the seeded state dicts of transformers' own modules; the CLIP forward with
`output_hidden_states`, the OWL-ViT `__call__` (not `detect()`: its host read of the counts would read memory no kernel
wrote) and the SAM `__call__` with box prompts and with point prompts (neither path reads a device result on the host,
so both are traced to their end).  Without transformers they print that they were skipped.  A scenario that raises is
reported with its exception and the run goes on.

The four `vae_*` scenarios trace the AutoencoderKL blocks on a small seeded `synth_aekl_state_dict`: `HipVAEDecoder.decode`
on a square and on a rectangular latent, `HipVAEEncoder.encode_moments`, and `HipVAE.encode` on a uint8 image.

Not seen: work torch does by itself (plain `tensor.copy_` of a call's state), and graph replay; the GPU tests that compare
graph replay with eager runs cover those.  The hashes change with every legitimate change of a plan or a tuning table:
this is a tool for comparing two trees, not a test, and no expected hash is kept.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch

# entry point -> index of its coefficient-table argument
STEP_TABLE_ARG = {"lgd_cfg_ddim_step_f32": 3, "lgd_cfg_multistep_step_f32": 4, "lgd_cfg_plms_step_f32": 5,
                  "lgd_cfg_lms_step_f32": 4,
                  "lgd_multidiffusion_step_f32": 7, "lgd_multidiffusion_views_f32": 9}


class Recorder:
    def __init__(self, ops):
        self.ops = ops
        self.log, self.names = [], {}
        self.keep, self.by_ptr = [], {}
        self._p, self._gemm_desc = ops._p, ops.gemm_desc
        ops._call = self.call
        ops._stream = lambda: C.c_void_p(0)
        ops._p = self.p
        ops.gemm_desc = self.gemm_desc
        ops.copy_ = self.copy_
        ops.zero_ = self.zero_

    # ---- keep-alive wrappers
    def hold(self, t):
        if torch.is_tensor(t):
            self.keep.append(t)
            self.by_ptr[t.data_ptr()] = t
        return t

    def p(self, t):
        return self._p(self.hold(t))

    def gemm_desc(self, *a, **k):
        for x in list(a) + list(k.values()):
            self.hold(x)
        return self._gemm_desc(*a, **k)

    def copy_(self, dst, src):
        self.log.append(f"copy_({self.ptr(self.hold(dst).data_ptr())},"
                        f"{self.ptr(self.hold(src).data_ptr()) if torch.is_tensor(src) else repr(src)},{dst.numel()})")
        return dst.copy_(src)

    def zero_(self, t):
        self.log.append(f"zero_({self.ptr(self.hold(t).data_ptr())},{t.numel()})")
        return t.zero_()

    # ---- the recorder
    def ptr(self, v):
        return "p%d" % self.names.setdefault(v, len(self.names)) if v else "null"

    def text(self, a):
        if isinstance(a, C.c_void_p):
            return self.ptr(a.value or 0)
        if hasattr(a, "_obj"):                                   # byref(LgdGemmDesc)
            d = a._obj
            return "desc(" + ",".join(self.ptr(getattr(d, f) or 0) if t is C.c_void_p else repr(getattr(d, f))
                                      for f, t in d._fields_) + ")"
        return repr(a)

    def call(self, name, *args):
        line = name + "(" + ",".join(self.text(a) for a in args) + ")"
        if name in STEP_TABLE_ARG:
            tab = self.by_ptr[args[STEP_TABLE_ARG[name]].value]
            line += " table=" + hashlib.sha256(tab.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
        self.log.append(line)

    def section(self, fn):
        self.names = {}
        n0 = len(self.log)
        fn()
        return self.log[n0:]


def scenarios(root):
    """name -> callable, in a fixed order; engines and samplers are shared like a process would share them."""
    sys.path.insert(0, root)
    import lgd_amd  # noqa: F401
    from lgd_amd import multidiffusion, ops, pipeline, sdxl, vae, weights
    from lgd_amd.sampler import Job, LMDSampler
    from lgd_amd.scheduler import DPMSolverMultistepScheduler, PNDMScheduler
    from lgd_amd.unet import UNetEngine
    rec = Recorder(ops)
    dev = torch.device("cpu")
    rnd = lambda seed, shape: torch.randn(shape, generator=torch.Generator().manual_seed(seed))

    cfg = weights.CONFIGS["tiny"]
    sm = LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)), use_graphs=False)
    unc, cond = weights.synth_embeddings(cfg, 1, seed=1)
    text = torch.cat([unc, cond])
    lat = rnd(0, (1, 4, 32, 32))
    guid = dict(bboxes=[[[0.1, 0.1, 0.5, 0.5]]], object_positions=[[1, 2]], max_index_step=2, max_iter=2,
                loss_threshold=-1.0)                              # a negative threshold keeps the guidance loop running
    hist = rnd(2, (5, 1, 4, 32, 32))
    fmask = torch.zeros((32, 32))
    fmask[8:20, 4:16] = 1

    P = 3
    masks = torch.zeros((P, 1, 32, 32))
    masks[1, :, :8] = 1
    masks[2, :, 20:] = 1
    masks[0] = 1 - masks[1] - masks[2]
    md_texts = rnd(3, (2 * P, 77, cfg.cross_attention_dim))
    md_bg = rnd(4, (2, 4, 32, 32))
    md_picks = torch.tensor([[0, 1], [1, 0]])

    xcfg = weights.CONFIGS["tiny_xl"]
    refiner = sdxl.SDXLRefiner(UNetEngine(xcfg, dev, weights.synth_state_dict(xcfg, 0), max_text_batch=2), None, None,
                               use_graphs=False)
    pe, pooled = rnd(5, (2, 77, xcfg.cross_attention_dim)), rnd(6, (2, xcfg.pooled_dim))

    gcfg = weights.CONFIGS["tiny_gligen"]
    gsm = LMDSampler(UNetEngine(gcfg, dev, weights.synth_state_dict(gcfg, 0)), use_graphs=False)
    boxes = [("a cat", [20, 40, 80, 100]), ("a dog", [140, 60, 80, 110])]
    boxes2 = [("a bird", [30, 30, 90, 70]), ("a tree", [130, 20, 100, 200])]
    glay = [pipeline.CachedLayout.synthetic(gcfg, b, index=i, height=256, width=256) for i, b in enumerate((boxes, boxes2))]
    lay = pipeline.CachedLayout.synthetic(cfg, boxes, height=256, width=256)
    small = dict(num_inference_steps=4, height=256, width=256, decode=False)

    vsd = vae.synth_aekl_state_dict((32, 32, 64, 64), 1, seed=1)
    vdec, venc, vpair = vae.HipVAEDecoder(vsd, dev), vae.HipVAEEncoder(vsd, dev), vae.HipVAE(vsd, dev)
    vimg = torch.randint(0, 256, (1, 32, 32, 3), generator=torch.Generator().manual_seed(10), dtype=torch.uint8)

    return rec, {
        "ddim": lambda: sm.denoise_batch([Job(lat, text)], 4),
        "pndm": lambda: sm.denoise_batch([Job(lat, text)], 4, scheduler=PNDMScheduler()),
        "dpm": lambda: sm.denoise_batch([Job(lat, text)], 4, scheduler=DPMSolverMultistepScheduler()),
        "guided": lambda: sm.denoise_batch([Job(lat, text, guidance=guid)], 4),
        "frozen_mask": lambda: sm.denoise_batch([Job(hist, text, frozen_mask=fmask)], 4, frozen_steps=2),
        "multidiffusion": lambda: multidiffusion.multidiffusion_generate(sm, md_texts, masks, lat, md_bg, md_picks, steps=4,
                                                                         n_boot=2, decode=False),
        "sdxl_refiner": lambda: refiner.refine_latents(lat, pe, pooled, first_index=6, num_inference_steps=10, height=256,
                                                       width=256),
        "lmd_plus": lambda: pipeline.lmd_plus_generate_batch(gsm, glay[:1], overall_max_index_step=2,
                                                             overall_loss_threshold=-1.0, **small),
        "lmd_plus_fast_two_layouts": lambda: pipeline.lmd_plus_generate_batch(
            gsm, glay, overall_max_index_step=2, overall_loss_threshold=-1.0, use_fast_schedule=True, **small),
        "lmd": lambda: pipeline.lmd_generate_batch(sm, [lay], max_index_step=2, overall_max_index_step=2,
                                                   loss_threshold=-1.0, overall_loss_threshold=-1.0, **small),
        "backward_guidance": lambda: pipeline.backward_guidance_generate_batch(sm, [lay], max_index_step=2,
                                                                               loss_threshold=-1.0, **small),
        "boxdiff": lambda: pipeline.boxdiff_generate_batch(sm, [lay], max_index_step=2, **small),
        # what bench.py --full times per kernel: every launch sequence the sampler hands out, run once
        "profile_passes": lambda: [fn() for _, _, _, fn in gsm.profile_passes(32, 4, True, main_batches=(1, 2),
                                                                             guide_batches=(1, 2))],
        "vae_decode": lambda: vdec.decode(rnd(7, (2, 4, 8, 8))),
        "vae_decode_rect": lambda: vdec.decode(rnd(8, (1, 4, 8, 16))),
        "vae_encode_moments": lambda: venc.encode_moments(rnd(9, (2, 3, 32, 32))),
        "vae_encode_u8": lambda: vpair.encode(vimg),
        **towers(root),
    }


def towers(root):
    """name -> callable for the CLIP, OWL-ViT and SAM towers, or name -> None without transformers."""
    try:
        import transformers
    except ImportError:
        return dict.fromkeys(("clip", "owlvit", "sam"))
    sys.path.insert(0, os.path.join(root, "tests"))
    import owl_detect_cases
    import sam_cases
    from lgd_amd import clip, owlvit, sam

    def run_clip():
        torch.manual_seed(0)
        hf = transformers.CLIPTextModel(transformers.CLIPTextConfig(
            vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
            max_position_embeddings=16, eos_token_id=2, bos_token_id=998, pad_token_id=0))
        ids = torch.randint(10, 998, (2, 16), generator=torch.Generator().manual_seed(1))
        clip.from_hf(hf, "cpu")(ids, output_hidden_states=True)

    def run_owlvit():
        cfg = owl_detect_cases.tiny_hf_config()
        torch.manual_seed(0)
        hf = owl_detect_cases.redraw_weights(transformers.OwlViTForObjectDetection(cfg), seed=3)
        pv, ids = owl_detect_cases.model_inputs(cfg, 2, 3, seed=4, zero_rows=(4,))
        owlvit.from_hf(hf, "cpu")(pixel_values=pv, input_ids=ids, attention_mask=(ids > 0).long())

    def run_sam():
        cfg = sam_cases.small_config(transformers)
        hf = sam_cases.build_hf(transformers, cfg)
        model = sam.HipSamModel(sam.SamConfig.from_hf(cfg), hf.state_dict(), device="cpu")
        for points in (False, True):
            model(**sam_cases.inputs(cfg, B=2, P=2, points=points))
    return {"clip": run_clip, "owlvit": run_owlvit, "sam": run_sam}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("root", nargs="?", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout to trace (the directory that holds lgd_amd.py)")
    ap.add_argument("--dump", metavar="DIR", help="write the full text of every scenario to DIR/<scenario>.txt")
    ap.add_argument("--only", nargs="+", metavar="NAME", help="run only these scenarios")
    args = ap.parse_args()
    rec, todo = scenarios(os.path.abspath(args.root))
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    for name, fn in todo.items():
        if args.only and name not in args.only:
            continue
        if fn is None:
            print(f"{name}: skipped (needs transformers)")
            continue
        try:
            lines = rec.section(fn)
        except Exception as e:
            print(f"{name}: raised {type(e).__name__}: {e}")
            continue
        body = "\n".join(lines) + "\n"
        print(f"{name}: {len(lines)} lines, sha256 {hashlib.sha256(body.encode()).hexdigest()[:16]}")
        if args.dump:
            with open(os.path.join(args.dump, name + ".txt"), "w") as fh:
                fh.write(body)


if __name__ == "__main__":
    main()
