"""Record which kernel v3d_gemm launches for every call of the project's workloads -> tests/golden/gemm_dispatch.json, the fixture that
tests/test_gemm_plan.py holds the (GPU-free) planner to.  Run it on the GPU at the commit whose choices are to be pinned: it needs only
HipOps.gemm / _gemm_args / last_gemm_launch and the two launch counters of the library.

  python tools/record_gemm_dispatch.py                 every workload below, one child process each, merged into tests/golden/gemm_dispatch.json
  python tools/record_gemm_dispatch.py --only model    one workload in this process (its V3D_GEMM_* / V3D_STREAMK settings come from the environment)

Workloads: `model` = one guided U-Net evaluation of the headline config (18 frames, 64 x 64 latents: all four levels), the 18-frame VAE decode,
the VAE encode, the CLIP ViT-H/14 tower, the frame-shard ranks with 3 and 2 local frames (8-GPU split of the 18 frames), and synthetic shapes
for kernels that valid arguments reach but the model does not; `scene` = one evaluation + decode at the scene config's size (24 frames,
72 x 128 latents); `ops` = every case of tests/op_cases.py that calls HipOps.gemm - once under the default policy and once under each forced
setting of tests/test_gemm_impls.py plus V3D_STREAMK=0 (the knobs are read once per process).

A row holds every non-pointer field of v3d_gemm_args, for every pointer None or its address modulo 256, the CU count, the five policy knobs
and what the library reports it launched: family, bm, bn, tiles, split-K ways, stream-K tail tiles (v3d_debug_last_gemm_launch), and whether
the stream-K / GroupNorm-epilogue launch counters moved."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.json")
OUT_DIR = os.path.join(ROOT, "build", "gemm_dispatch")      # the children's row files (build/ is not tracked)
KNOBS = ("V3D_GEMM_IMPL", "V3D_GEMM_SPLITK", "V3D_GEMM_V3S", "V3D_GEMM_V6", "V3D_STREAMK")
KNOB_DEFAULTS = (0, -1, 2, 1, 1)                 # (gemm.hip GemmPolicy)
LAUNCH = ("family", "bm", "bn", "tiles", "splitk", "streamk_tail", "streamk_launch", "gn_epilogue_launch")
# (workload, environment): the forced settings are those of tests/test_gemm_impls.py + the stream-K switch
JOBS = [("model", {}), ("scene", {}), ("ops", {}),
        ("ops", {"V3D_GEMM_IMPL": "1"}), ("ops", {"V3D_GEMM_IMPL": "2"}), ("ops", {"V3D_GEMM_IMPL": "3"}),
        ("ops", {"V3D_GEMM_IMPL": "2", "V3D_GEMM_SPLITK": "3"}), ("ops", {"V3D_GEMM_IMPL": "3", "V3D_GEMM_V3S": "0"}),
        ("ops", {"V3D_GEMM_V6": "2"}), ("ops", {"V3D_STREAMK": "0"})]


def policy():
    return [int(os.environ[k]) if os.environ.get(k) else d for k, d in zip(KNOBS, KNOB_DEFAULTS)]


def fields():
    from v3d_amd.hip import _GemmArgs, c_vp
    ptrs = [n for n, t in _GemmArgs._fields_ if t is c_vp]
    vals = [n for n, t in _GemmArgs._fields_ if t is not c_vp]
    return ptrs, vals


def install(rows: dict):
    """HipOps.gemm -> the same call, recorded (rows: key -> row; identical calls collapse)."""
    from v3d_amd.hip import HipOps
    ptrs, vals = fields()
    pol = policy()

    def counter(hip, name):
        fn = getattr(hip.lib, name)
        fn.restype, fn.argtypes = C.c_longlong, []
        return int(fn())

    def gemm(self, g):
        if self._gemm_in_row_chunks(g):          # (re-enters this function once per chunk)
            return
        a = self._gemm_args(g)
        sk0, gn0 = counter(self, "v3d_debug_sk_launches"), counter(self, "v3d_debug_gn_epilogue_launches")
        self._check(self.lib.v3d_gemm(C.byref(a), self._stream()), "v3d_gemm")
        rec = self.last_gemm_launch()
        launch = [rec["family"], rec["bm"], rec["bn"], rec["tiles"], rec["splitk"], rec["streamk_tail"],
                  int(counter(self, "v3d_debug_sk_launches") > sk0), int(counter(self, "v3d_debug_gn_epilogue_launches") > gn0)]
        row = {"ptr": [None if not getattr(a, n) else int(getattr(a, n)) % 256 for n in ptrs], "val": [getattr(a, n) for n in vals],
               "cus": rec["cus"], "policy": pol, "launch": launch}
        row["val"] = [float("%.6g" % v) if isinstance(v, float) else v for v in row["val"]]      # (c_acc / c_res*: fp32 values, not their double expansion)
        rows[json.dumps(row, sort_keys=True)] = row

    HipOps.gemm = gemm


def run_model(scene: bool):
    import torch
    import bench
    from v3d_amd import synth
    from v3d_amd.dist import SimFrameShard, sharded_sample
    dev = "cuda"
    T, H, W = (24, 72, 128) if scene else (bench.T_FRAMES, bench.LAT, bench.LAT)
    unet, wrapped, dec, _, denoiser = bench.build_models(dev, frames=T)
    noise, c, uc = synth.synthetic_conditioning(T, H, W, seed=23, device=dev)
    extra = {"image_only_indicator": torch.zeros(2, T, device=dev), "num_video_frames": T}
    cond = {k: torch.cat([uc[k], c[k]]) for k in c}
    denoiser(wrapped, torch.cat([noise, noise]), torch.full((2 * T,), 10.0, device=dev), cond, **extra)
    dec(torch.randn(T, 4, H, W, device=dev), timesteps=T)
    torch.cuda.synchronize()
    if scene:
        return
    # frame shard: the rank with the most (3) and the fewest (2) of the 18 frames on 8 GPUs, one EDM step + the local decode
    from v3d_amd.sgm.modules.diffusionmodules.sampling import EulerEDMSampler
    P = bench.P
    for rank in (0, 7):
        sh = SimFrameShard(T, 8, rank)
        smp = EulerEDMSampler(discretization_config={"target": P + "discretizer.EDMDiscretization", "params": {"sigma_max": 700.0}}, num_steps=1,
                              guider_config={"target": P + "guiders.LinearPredictionGuider", "params": {"max_scale": bench.CFG, "min_scale": bench.CFG, "num_frames": T}},
                              device=dev)
        sharded_sample(sh, smp, denoiser, wrapped, lambda z: dec(z * (1.0 / 0.18215), timesteps=sh.T_local), noise.clone(), c, uc, B=1, gather=False)
        torch.cuda.synchronize()
    del unet, wrapped, dec
    torch.cuda.empty_cache()
    from v3d_amd.sgm.modules.diffusionmodules.model import Encoder
    with torch.device(dev):
        enc = Encoder(**synth.encoder_config(128)).eval()
    synth.init_module_fast(enc, seed=3)
    enc(torch.rand(1, 3, 512, 512, device=dev) * 2 - 1)
    from v3d_amd.sgm.modules.encoders.modules import FrozenOpenCLIPImageEmbedder
    clip = FrozenOpenCLIPImageEmbedder(freeze=True).eval().to(dev)
    clip(torch.rand(1, 3, 512, 512, device=dev) * 2 - 1)
    torch.cuda.synchronize()
    synthetic(dev)


def synthetic(dev):
    """Kernels the model never reaches but valid arguments do."""
    import torch
    from v3d_amd.ops import GEMM_CONV3X3, GemmCall, get_ops
    ops = get_ops()
    BF = torch.bfloat16

    def conv(n_img, H, W, N, K):
        M = n_img * H * W
        ops.gemm(GemmCall(A=torch.zeros(M, K, dtype=BF, device=dev), W=torch.zeros(9, N, K, dtype=BF, device=dev), out=torch.zeros(M, N, dtype=BF, device=dev),
                          M=M, N=N, K=K, mode=GEMM_CONV3X3, Hin=H, Win=W, Hout=H, Wout=W, stride=1, up=1))

    def lin(M, N, K):
        ops.gemm(GemmCall(A=torch.zeros(M, K, dtype=BF, device=dev), W=torch.zeros(1, N, K, dtype=BF, device=dev), out=torch.zeros(M, N, dtype=BF, device=dev), M=M, N=N, K=K))

    conv(4, 16, 16, 128, 160)        # 45 stages of 32 with K % 64 != 0: the 128 x 128 tile on four 32-deep stages
    conv(36, 8, 8, 128, 160)
    lin(512, 128, 2080)              # the same kernel from a linear: 65 stages
    lin(1024, 128, 2048)             # 64 stages, K % 64 == 0, too many tiles to split: two 64-deep stages
    lin(256, 128, 40)                # K % 32 != 0: the register-staged kernel
    lin(4096, 320, 96)               # 64-wide tiles, K % 64 != 0
    torch.cuda.synchronize()


def run_ops():
    import torch
    import op_cases
    from v3d_amd.ops import get_ops
    hip = get_ops()

    class NoEmu:                     # the cases' reference side is not needed here (their own tests check it): the launches are what is recorded
        def __getattr__(self, name):
            return lambda *a, **k: None

    calling = (op_cases.case_gemm, op_cases.case_conv_gn, op_cases.case_convt3_split_halo)
    for name, fn, kw, _ in op_cases.all_cases(full=True):
        if fn not in calling:
            continue
        try:
            fn(hip, NoEmu(), "cuda", **kw)
        except AssertionError as e:          # (assertions against the absent reference / expectations that hold under the default policy only)
            print(f"[record] {name}: {str(e)[:100]}", flush=True)
        torch.cuda.synchronize()
    synthetic("cuda")


def child(only: str, out_path: str):
    import torch
    torch.set_grad_enabled(False)
    rows = {}
    install(rows)
    {"model": lambda: run_model(False), "scene": lambda: run_model(True), "ops": run_ops}[only]()
    from v3d_amd.ops import get_ops
    get_ops().check_health()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(list(rows.values()), open(out_path, "w"))
    print(f"[record] {only} {policy()}: {len(rows)} distinct calls -> {out_path}", flush=True)


def merge(paths):
    ptrs, vals = fields()
    seen, rows = set(), []
    for p in paths:
        for r in json.load(open(p)):
            k = json.dumps(r, sort_keys=True)
            if k not in seen:
                seen.add(k)
                rows.append(r)
    rows.sort(key=lambda r: (r["policy"], r["launch"], json.dumps(r["val"])))
    with open(FIXTURE, "w") as f:
        f.write('{"knobs": %s,\n "pointers": %s,\n "values": %s,\n "launch": %s,\n "rows": [\n' % tuple(json.dumps(list(x)) for x in (KNOBS, ptrs, vals, LAUNCH)))
        f.write(",\n".join("  " + json.dumps([r["cus"], r["policy"], r["ptr"], r["val"], r["launch"]], separators=(",", ":")) for r in rows))
        f.write("\n ]}\n")
    print(f"[record] {len(rows)} rows -> {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")


def main():
    if "--only" in sys.argv:
        child(sys.argv[sys.argv.index("--only") + 1], sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(OUT_DIR, "one.json"))
        return
    if "--merge" in sys.argv:
        merge(sys.argv[sys.argv.index("--merge") + 1:])
        return
    paths = []
    for i, (only, env) in enumerate(JOBS):
        out = os.path.join(OUT_DIR, f"{i:02d}_{only}.json")
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", only, "--out", out], env=dict(e, **env), timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"workload {only} {env} failed with status {r.returncode}: nothing after it was started")
        paths.append(out)
    merge(paths)


if __name__ == "__main__":
    main()
