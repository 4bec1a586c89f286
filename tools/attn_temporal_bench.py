"""Temporal attention at the V3D_512 shapes: time per launch and effective HBM rate (q, k, v read + out written once).
python tools/attn_temporal_bench.py [T ...]: frame counts (default 18; T > 32 runs the long kernel)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from v3d_amd.ops import get_ops
torch.set_grad_enabled(False)
ops = get_ops()
dev = "cuda"
frames = [int(a) for a in sys.argv[1:]] or [18]
for (B, T, S, C) in [(b, t, s, c) for t in frames for (b, s, c) in [(2, 4096, 320), (2, 1024, 640), (2, 256, 1280), (2, 64, 1280), (8, 4096, 320)]]:
    heads = C // 64
    g = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(B, T, S, 3 * C, device=dev, generator=g).to(torch.bfloat16)
    out = torch.empty(B, T, S, C, device=dev, dtype=torch.bfloat16)
    f = lambda: ops.attn_temporal(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], out, heads, 0.125)
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / n * 1e3
    byts = B * T * S * C * 2 * 4
    print(f"attn_temporal B={B} T={T} S={S:5d} C={C:5d}  {us:8.1f} us  {byts / us / 1e6:6.2f} TB/s  checksum {out.float().abs().mean().item():.6f}")
