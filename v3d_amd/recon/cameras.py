"""Orbit cameras of a generated V3D video, restated from the geometry the reference's reconstruction uses (recon/utils/camera_utils.py,
recon/scene/dataset_readers.py, recon/scene/cameras.py).

Camera k of T sits at azimuth 360 k / T degrees, a fixed elevation and distance from the origin, +z up, and looks at the origin with OpenCV
axes (x right, y down, z forward).  Matrices use the row-vector convention: p_view = [x y z 1] @ world_view, p_clip = [x y z 1] @ full_proj.
Everything is evaluated in float64 and stored as float32."""
from __future__ import annotations

import dataclasses
import math
from typing import List

import numpy as np
import torch

ZNEAR, ZFAR = 0.01, 100.0


@dataclasses.dataclass
class Camera:
    world_view: torch.Tensor      # [4, 4] fp32, row-vector convention
    full_proj: torch.Tensor       # [4, 4] fp32
    center: torch.Tensor          # [3] fp32
    fovx: float
    fovy: float
    width: int
    height: int

    @property
    def tanfovx(self) -> float:
        return math.tan(self.fovx * 0.5)

    @property
    def tanfovy(self) -> float:
        return math.tan(self.fovy * 0.5)


def orbit_positions(num_frames: int, radius: float, elevation: float) -> np.ndarray:
    """[T, 3] float64 camera centres on the orbit."""
    el = math.radians(elevation)
    az = np.arange(num_frames, dtype=np.float64) * (2.0 * math.pi / num_frames)
    return radius * np.stack([math.cos(el) * np.cos(az), math.cos(el) * np.sin(az), np.full_like(az, math.sin(el))], axis=1)


def view_matrix(eye: np.ndarray) -> np.ndarray:
    """Row-vector world -> view matrix [4, 4] (float64) of a camera at `eye` looking at the origin with +z up: the view axes are
    forward = -eye / |eye|, right = forward x up (normalised), down = forward x right; p_view = R (p - eye)."""
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])          # rows: view axes in world coordinates
    M = np.eye(4)
    M[:3, :3] = R.T                           # row-vector form: [p 1] @ M = R p + t
    M[3, :3] = -R @ eye
    return M


def perspective(fovx: float, fovy: float, znear: float = ZNEAR, zfar: float = ZFAR) -> np.ndarray:
    """Row-vector view -> clip matrix [4, 4] (float64): x / tan(fovx/2), y / tan(fovy/2), depth mapped to [0, 1] over [znear, zfar], w = z."""
    P = np.zeros((4, 4))
    P[0, 0] = 1.0 / math.tan(fovx / 2)
    P[1, 1] = 1.0 / math.tan(fovy / 2)
    P[2, 2] = zfar / (zfar - znear)
    P[3, 2] = -zfar * znear / (zfar - znear)
    P[2, 3] = 1.0
    return P


def make_camera(eye: np.ndarray, fovx: float, fovy: float, width: int, height: int, device="cpu") -> Camera:
    V = view_matrix(eye)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=device)  # noqa: E731
    return Camera(f32(V), f32(V @ perspective(fovx, fovy)), f32(eye), fovx, fovy, int(width), int(height))


def orbit_cameras(num_frames: int, radius: float = 2.0, elevation: float = 0.0, fov: float = 60.0, reso: int = 512, device="cpu"):
    """Returns (cameras, cameras_extent): square reso x reso views with fov degrees on both axes; cameras_extent = 1.1 x the largest distance of
    a camera centre from the centres' mean (the reference's scene radius)."""
    eyes = orbit_positions(num_frames, radius, elevation)
    fovr = math.radians(fov)
    cams: List[Camera] = [make_camera(e, fovr, fovr, reso, reso, device) for e in eyes]
    extent = 1.1 * float(np.linalg.norm(eyes - eyes.mean(axis=0), axis=1).max())
    return cams, extent
