"""Frame-sharded ancestral sampling on CPU: two gloo processes, exact-mode emulated backend (tests/sampler_emul.py), T = 3 frames split 2 + 1.
Each rank seeds torch DIFFERENTLY, so the seed agreement of `sharded_sample` is exercised: the sharded result must equal the unsharded run
that draws rank 0's seed, within the sharding tolerance of tests/test_dist_gloo.py."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tiny import TINY, build_denoiser, build_unet, tiny_unet_inputs

KINDS = ("EulerAncestralSampler", "DPMPP2SAncestralSampler")
STEPS = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    torch.set_grad_enabled(False)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sampler_emul import SamplerEmulOps
        from test_samplers_emul import make_sampler
        from v3d_amd.dist import FrameShard, sharded_sample
        from v3d_amd.ops import use_backend
        from v3d_amd.sgm.modules.diffusionmodules.wrappers import OpenAIWrapper
        p = TINY
        T = p["T"]
        sh = FrameShard(T)
        noise, c, uc, *_ = tiny_unet_inputs(T, p["H"], p["W"], p["seed"])
        errs = {}
        with use_backend(SamplerEmulOps("cpu", exact=True)):
            net = build_unet()
            den, wr = build_denoiser(), OpenAIWrapper(net)
            for kind in KINDS:
                key = {"EulerAncestralSampler": "euler_ancestral", "DPMPP2SAncestralSampler": "dpmpp2s_ancestral"}[kind]
                smp = make_sampler(key, STEPS)
                torch.manual_seed(100 + rank)                  # ranks' generators differ: rank 0's draw must win
                zs = sharded_sample(sh, smp, den, wr, lambda zz: zz, noise.clone(), c, uc, B=1)
                assert smp.noise_seed is None and smp.noise_frames is None      # the caller's sampler is untouched
                torch.manual_seed(100)                          # the unsharded run of rank 0's generator state
                extra = {"image_only_indicator": torch.zeros(2, T), "num_video_frames": T}
                z = make_sampler(key, STEPS)(lambda i, s, cc: den(wr, i, s, cc, **extra), noise.clone(), cond=c, uc=uc)
                errs[kind] = ((zs - z).abs().max() / z.abs().max()).item()
                torch.manual_seed(101)
                zo = make_sampler(key, STEPS)(lambda i, s, cc: den(wr, i, s, cc, **extra), noise.clone(), cond=c, uc=uc)
                errs[kind + "_other_seed"] = ((zo - z).abs().max() / z.abs().max()).item()
        q.put((rank, sh.T_local, errs))
    except Exception as e:  # report instead of leaving the parent waiting on the queue
        import traceback
        q.put((rank, -1, traceback.format_exc(), str(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_two_rank_ancestral_samplers_match_unsharded():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for pr in procs:
        pr.join(timeout=60)
    for r in res:
        assert r[1] >= 0, f"rank {r[0]} failed:\n{r[2]}"
    res.sort(key=lambda r: r[0])
    assert [r[1] for r in res] == [2, 1]
    for rank, _, errs in res:
        for kind in KINDS:
            assert errs[kind] <= 5e-5, f"rank {rank}: sharded {kind} differs from the unsharded run of rank 0's seed: {errs[kind]}"
            assert errs[kind + "_other_seed"] > 1e-3, f"rank {rank}: {kind}: another seed should give other latents"
