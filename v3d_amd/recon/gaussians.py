"""3-D Gaussian parameters, densification and PLY I/O (reference: recon/scene/gaussian_model.py).

Parameters are stored pre-activation, as in the reference: xyz, SH degree-0 features [P, 1, 3] (features_rest [P, 0, 3]), log scales,
unnormalised quaternions (w, x, y, z) and opacity logits.  Adam (eps 1e-15), the row surgery on its state and the index / concatenation work
of densification are torch plumbing on whatever device the parameters live on; the CPU tests drive the same code."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn

SH_C0 = 0.28209479177387814


def rgb_to_sh(rgb):
    return (rgb - 0.5) / SH_C0


def sh_to_rgb(sh):
    return sh * SH_C0 + 0.5


def quat_to_rot(r: torch.Tensor) -> torch.Tensor:
    q = r / torch.sqrt((r * r).sum(dim=1, keepdim=True))
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


class ExponentialDecay:
    """Learning rate that falls geometrically from `start` (step 0) to `end` (step `steps`) and stays there; with warmup_steps > 0 it is
    additionally scaled by a quarter sine wave that rises from warmup_mult to 1 over the first warmup_steps steps.  Negative steps and an
    all-zero schedule give 0.  (The reference's xyz schedule, get_expon_lr_func, uses no warm-up.)"""

    def __init__(self, start: float, end: float, steps: int, warmup_steps: int = 0, warmup_mult: float = 1.0):
        self.start, self.end, self.steps = float(start), float(end), steps
        self.warmup_steps, self.warmup_mult = warmup_steps, warmup_mult

    def __call__(self, step: int) -> float:
        if step < 0 or self.start == self.end == 0.0:
            return 0.0
        frac = min(1.0, max(0.0, step / self.steps))
        lr = math.exp(math.log(self.start) + frac * (math.log(self.end) - math.log(self.start)))
        if self.warmup_steps > 0:
            ramp = math.sin(0.5 * math.pi * min(1.0, step / self.warmup_steps))
            lr *= self.warmup_mult + (1.0 - self.warmup_mult) * ramp
        return lr


class GaussianModel:
    def __init__(self, sh_degree: int = 0):
        if sh_degree != 0:
            raise NotImplementedError(f"sh_degree {sh_degree}: only SH degree 0 is implemented (the command V3D documents passes --sh_degree 0)")
        self.sh_degree = 0
        self.xyz = self.features_dc = self.features_rest = self.scaling = self.rotation = self.opacity = None
        self.optimizer: Optional[torch.optim.Adam] = None
        self.percent_dense = 0.0
        self.spatial_lr_scale = 0.0
        self.generator: Optional[torch.Generator] = None

    # ---- construction ------------------------------------------------------------------------
    def set_params(self, xyz, features_dc, scaling, rotation, opacity):
        P = xyz.shape[0]
        self.xyz = nn.Parameter(xyz.float().contiguous())
        self.features_dc = nn.Parameter(features_dc.float().reshape(P, 1, 3).contiguous())
        self.features_rest = nn.Parameter(torch.zeros(P, 0, 3, device=xyz.device))
        self.scaling = nn.Parameter(scaling.float().contiguous())
        self.rotation = nn.Parameter(rotation.float().contiguous())
        self.opacity = nn.Parameter(opacity.float().reshape(P, 1).contiguous())
        self._reset_stats()

    def create_from_points(self, xyz: torch.Tensor, colors: torch.Tensor, spatial_lr_scale: float, dist2: Optional[torch.Tensor] = None,
                           init_opacity: float = 0.5):
        """Initialisation of the reference's create_from_pcd: SH from the point colours, isotropic log scale from the mean squared distance
        to the 3 nearest neighbours (the exact gs_knn3 kernel when dist2 is not given), identity rotation, opacity logit of init_opacity."""
        self.spatial_lr_scale = spatial_lr_scale
        if dist2 is None:
            from ..ops import get_ops
            dist2 = get_ops().gs_knn3(xyz.float().contiguous())
        P = xyz.shape[0]
        log_scale = 0.5 * torch.log(dist2.clamp(min=1e-7))                   # log of the RMS neighbour distance, on all three axes
        identity = torch.tensor([1.0, 0.0, 0.0, 0.0], device=xyz.device).expand(P, 4)
        self.set_params(xyz, rgb_to_sh(colors.float()), log_scale.unsqueeze(1).expand(P, 3), identity,
                        torch.logit(torch.full((P, 1), init_opacity, device=xyz.device)))

    def _reset_stats(self):
        P, d = self.xyz.shape[0], self.xyz.device
        self.xyz_gradient_accum = torch.zeros(P, 1, device=d)
        self.denom = torch.zeros(P, 1, device=d)
        self.max_radii2D = torch.zeros(P, device=d)

    def params(self) -> Dict[str, nn.Parameter]:
        return {"xyz": self.xyz, "f_dc": self.features_dc, "f_rest": self.features_rest, "opacity": self.opacity, "scaling": self.scaling,
                "rotation": self.rotation}

    def _set(self, d: Dict[str, torch.Tensor]):
        self.xyz, self.features_dc, self.features_rest = d["xyz"], d["f_dc"], d["f_rest"]
        self.opacity, self.scaling, self.rotation = d["opacity"], d["scaling"], d["rotation"]

    def training_setup(self, opt, seed: int = 0):
        """Adam (eps 1e-15) with one named group per parameter at the reference's learning rates; the xyz rate follows an exponential
        decay over position_lr_max_steps, scaled by the scene extent.  `seed` seeds the generator of the split samples."""
        self.percent_dense = opt.percent_dense
        self._reset_stats()
        lrs = {"xyz": opt.position_lr_init * self.spatial_lr_scale, "f_dc": opt.feature_lr, "f_rest": opt.feature_lr / 20.0,
               "opacity": opt.opacity_lr, "scaling": opt.scaling_lr, "rotation": opt.rotation_lr}
        p = self.params()
        self.optimizer = torch.optim.Adam([{"params": [p[k]], "lr": lr, "name": k} for k, lr in lrs.items()], lr=0.0, eps=1e-15)
        self.xyz_lr = ExponentialDecay(opt.position_lr_init * self.spatial_lr_scale, opt.position_lr_final * self.spatial_lr_scale,
                                       opt.position_lr_max_steps)
        self.generator = torch.Generator(device=self.xyz.device).manual_seed(seed)

    def update_learning_rate(self, iteration: int) -> float:
        lr = self.xyz_lr(iteration)
        for g in self.optimizer.param_groups:
            if g["name"] == "xyz":
                g["lr"] = lr
        return lr

    # ---- activations -------------------------------------------------------------------------
    @property
    def get_scaling(self):
        return torch.exp(self.scaling)

    @property
    def get_opacity(self):
        return torch.sigmoid(self.opacity)

    # ---- optimizer surgery -------------------------------------------------------------------
    def _rebuild(self, values: Dict[str, torch.Tensor], moments):
        """Swap each parameter named in `values` for a new leaf holding that tensor, and carry its Adam state over: both moment tensors go
        through moments(old_moment, new_param); the step count stays."""
        current = {}
        for group in self.optimizer.param_groups:
            name, old = group["name"], group["params"][0]
            if name in values:
                new = nn.Parameter(values[name].detach().contiguous())
                state = self.optimizer.state.pop(old, None)
                if state is not None:
                    for key in ("exp_avg", "exp_avg_sq"):
                        state[key] = moments(state[key], new)
                    self.optimizer.state[new] = state
                group["params"] = [new]
                old = new
            current[name] = old
        self._set(current)

    def prune_points(self, drop: torch.Tensor):
        keep = ~drop
        self._rebuild({k: v.detach()[keep] for k, v in self.params().items()}, lambda m, _new: m[keep])
        self.xyz_gradient_accum, self.denom, self.max_radii2D = self.xyz_gradient_accum[keep], self.denom[keep], self.max_radii2D[keep]

    # ---- densification -----------------------------------------------------------------------
    def _grow(self, clone: torch.Tensor, split: torch.Tensor, N: int):
        """New parameter rows: the Gaussians not split, then a copy of every `clone` one, then N children of every `split` one (child k of
        every parent before child k + 1).  A child sits at the parent's centre plus R (s * z), z ~ N(0, I) from the seeded generator, with the
        parent's scales divided by 0.8 N.  Adam moments: kept for the surviving rows, zero for the new ones.  Statistics restart."""
        p = {k: v.detach() for k, v in self.params().items()}
        s = self.get_scaling.detach()[split]
        z = torch.randn((N,) + tuple(s.shape), generator=self.generator, device=s.device)
        offsets = torch.einsum("kij,nkj->nki", quat_to_rot(p["rotation"][split]), z * s)
        children = {k: v[split].repeat((N,) + (1,) * (v.dim() - 1)) for k, v in p.items()}
        children["xyz"] = (p["xyz"][split].unsqueeze(0) + offsets).reshape(-1, 3)
        children["scaling"] = torch.log(s / (0.8 * N)).repeat(N, 1)
        keep = ~split
        n_keep = int(keep.sum())
        self._rebuild({k: torch.cat((v[keep], v[clone], children[k])) for k, v in p.items()},
                      lambda m, new: torch.cat((m[keep], m.new_zeros((new.shape[0] - n_keep,) + tuple(m.shape[1:])))))
        self._reset_stats()

    def densify_and_prune(self, grad_threshold: float, min_opacity: float, extent: float, max_screen_size, N: int = 2):
        """Gaussians whose mean screen-space gradient since the last densification reaches grad_threshold grow: small ones (largest scale
        <= percent_dense * extent) are cloned, large ones split in N.  Then Gaussians below min_opacity are dropped and, with max_screen_size,
        also those larger than 0.1 * extent in the world.  The screen-size rule reads the statistics the growth step has just restarted, so
        (as in the reference's densify_and_prune) it removes nothing.  Returns the (clone, split) masks over the Gaussians before growth."""
        with torch.no_grad():
            ratio = (self.xyz_gradient_accum / self.denom).squeeze(1)
            ratio = ratio.masked_fill(ratio.isnan(), 0.0)        # never seen: no gradient
            hot = ratio >= grad_threshold
            large = self.get_scaling.max(dim=1).values > self.percent_dense * extent
            clone, split = hot & ~large, hot & large
            self._grow(clone, split, N)
            drop = self.get_opacity.squeeze(1) < min_opacity
            if max_screen_size:
                drop = drop | (self.max_radii2D > max_screen_size) | (self.get_scaling.max(dim=1).values > 0.1 * extent)
            self.prune_points(drop)
        return clone, split

    def record_view(self, radii: torch.Tensor, screen_grad: torch.Tensor):
        """Densification statistics of one rendered view: every Gaussian on screen (radius > 0) updates its largest screen radius and adds
        the norm of its NDC mean gradient to a running sum with a count."""
        seen = radii > 0
        self.max_radii2D = torch.where(seen, torch.maximum(self.max_radii2D, radii.float()), self.max_radii2D)
        self.xyz_gradient_accum += torch.where(seen, screen_grad[:, :2].norm(dim=1), 0.0).unsqueeze(1)
        self.denom += seen.float().unsqueeze(1)

    def reset_opacity(self):
        """Cap every opacity at 0.01 and restart its Adam moments."""
        capped = torch.clamp(self.get_opacity.detach(), max=0.01)
        self._rebuild({"opacity": torch.logit(capped)}, lambda _m, new: torch.zeros_like(new))

    # ---- PLY ---------------------------------------------------------------------------------
    def attribute_names(self) -> List[str]:
        names = ["x", "y", "z", "nx", "ny", "nz"]
        names += [f"f_dc_{i}" for i in range(self.features_dc.shape[1] * self.features_dc.shape[2])]
        names += [f"f_rest_{i}" for i in range(self.features_rest.shape[1] * self.features_rest.shape[2])]
        names += ["opacity"] + [f"scale_{i}" for i in range(self.scaling.shape[1])] + [f"rot_{i}" for i in range(self.rotation.shape[1])]
        return names

    def save_ply(self, path: str):
        P = self.xyz.shape[0]
        cols = [self.xyz.detach(), torch.zeros(P, 3, device=self.xyz.device), self.features_dc.detach().transpose(1, 2).flatten(1),
                self.features_rest.detach().transpose(1, 2).flatten(1), self.opacity.detach(), self.scaling.detach(), self.rotation.detach()]
        write_ply(path, self.attribute_names(), torch.cat(cols, 1).float().cpu().numpy())

    def load_ply(self, path: str, device="cpu"):
        names, data = read_ply(path)
        col = {n: data[:, i] for i, n in enumerate(names)}
        t = lambda keys: torch.tensor(np.stack([col[k] for k in keys], 1), dtype=torch.float32, device=device)  # noqa: E731
        if any(n.startswith("f_rest_") for n in names):
            raise NotImplementedError("PLY holds SH degree > 0 features; only degree 0 is implemented")
        self.set_params(t(["x", "y", "z"]), t(["f_dc_0", "f_dc_1", "f_dc_2"]), t(["scale_0", "scale_1", "scale_2"]),
                        t(["rot_0", "rot_1", "rot_2", "rot_3"]), t(["opacity"]))


def write_ply(path: str, names: List[str], data: np.ndarray):
    """Binary little-endian PLY with one `vertex` element of float properties (the layout plyfile writes for the reference)."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    data = np.ascontiguousarray(data, dtype="<f4")
    if data.ndim != 2 or data.shape[1] != len(names):
        raise ValueError(f"write_ply: data {data.shape} does not match {len(names)} attributes")
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {data.shape[0]}"] + [f"property float {n}" for n in names] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(data.tobytes())


def read_ply(path: str):
    """(attribute names, float32 [N, k]) of a binary little-endian PLY whose only element is `vertex` with float properties."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = raw[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary little-endian PLY is supported")
    n, names = None, []
    for ln in lines:
        p = ln.split()
        if p[:2] == ["element", "vertex"]:
            n = int(p[2])
        elif p[:1] == ["element"]:
            raise ValueError(f"{path}: unexpected element {p[1]}")
        elif p[:1] == ["property"]:
            if p[1] not in ("float", "float32"):
                raise ValueError(f"{path}: property {p[-1]} is {p[1]}, only float is supported")
            names.append(p[2])
    body = raw[end + len(b"end_header\n"):]
    data = np.frombuffer(body, dtype="<f4", count=n * len(names)).reshape(n, len(names))
    return names, data.astype(np.float32)
