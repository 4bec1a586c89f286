"""Image -> orbit -> 3-D Gaussians: the reconstruction step of V3D (the reference's recon/train_from_vid.py) on the gfx950 splat kernels
(csrc/gs.hip).  cameras: the orbit camera set; rasterize: the autograd rasterizer and fused loss; gaussians: parameters, densification,
PLY I/O; train: the optimisation loop."""
