"""The ancestral / DPM++ / linear-multistep samplers (v3d_amd/sgm/modules/diffusionmodules/sampling.py) on CPU, with the exact-fp32 emulated
backend plus the two sampler-loop ops (tests/sampler_emul.py), against fixtures the reference's own samplers produced over the tiny network
(tools/gen_golden_samplers.py: noise_sampler = the numpy restatement of the device noise, seed 1234)."""
import inspect
import os

import pytest
import torch

from conftest import ROOT, rel_cos
from sampler_emul import SamplerEmulOps, randn_ref
from tiny import P, TINY, build_denoiser, build_unet, tiny_unet_inputs
from v3d_amd.ops import use_backend
from v3d_amd.sgm.modules.diffusionmodules import sampling
from v3d_amd.sgm.modules.diffusionmodules.sampling_utils import get_ancestral_step, linear_multistep_coeff
from v3d_amd.sgm.modules.diffusionmodules.wrappers import OpenAIWrapper

torch.set_grad_enabled(False)

KINDS = {"euler_ancestral": ("EulerAncestralSampler", {"eta": 1.0}), "dpmpp2s_ancestral": ("DPMPP2SAncestralSampler", {"eta": 1.0}),
         "dpmpp2m": ("DPMPP2MSampler", {}), "lms": ("LinearMultistepSampler", {"order": 4})}


@pytest.fixture(scope="module")
def fixture():
    return torch.load(os.path.join(ROOT, "tests", "golden", "v3d_samplers.pt"))


def disc_config():
    return {"target": P + "discretizer.EDMDiscretization", "params": {"sigma_max": TINY["sigma_max"]}}


def make_sampler(kind, steps, guided=True, **kw):
    cls, params = KINDS[kind]
    g = None
    if guided:
        g = {"target": P + "guiders.LinearPredictionGuider",
             "params": {"max_scale": TINY["max_scale"], "min_scale": TINY["min_scale"], "num_frames": TINY["T"]}}
    return getattr(sampling, cls)(discretization_config=disc_config(), num_steps=steps, guider_config=g, device="cpu", **params, **kw)


def run_tiny(sampler, net, device="cpu"):
    """The sampler over the tiny network (fixture inputs); returns (latents, denoiser calls)."""
    p = TINY
    T = p["T"]
    noise, c, uc, *_ = tiny_unet_inputs(T, p["H"], p["W"], p["seed"])
    den, wr = build_denoiser(), OpenAIWrapper(net)
    ioi = torch.zeros(2, T, device=device)
    calls = [0]

    def f(inp, sigma, cc):
        calls[0] += 1
        return den(wr, inp, sigma, cc, image_only_indicator=ioi, num_video_frames=T)

    z = sampler(f, noise.to(device), cond={k: v.to(device) for k, v in c.items()}, uc={k: v.to(device) for k, v in uc.items()})
    return z, calls[0]


@pytest.fixture(scope="module")
def emul_net():
    with use_backend(SamplerEmulOps("cpu", exact=True)):
        yield build_unet()


@pytest.mark.parametrize("kind", list(KINDS))
def test_sampler_matches_reference_fixture(fixture, emul_net, kind):
    with use_backend(SamplerEmulOps("cpu", exact=True)):
        kw = {"noise_seed": fixture["seed"]} if kind.endswith("ancestral") else {}
        z, calls = run_tiny(make_sampler(kind, fixture["steps"], **kw), emul_net)
    rel, cos = rel_cos(z, fixture["z"][kind])
    assert rel <= 1e-4 and cos >= 0.99999, (kind, rel, cos)
    assert calls == fixture["calls"][kind], (kind, calls)


def cheap_run(sampler, seed_torch=None, steps=4):
    """The sampler over a frame-local stand-in denoiser (IdentityGuider): fast, and enough to see the noise."""
    x = torch.randn(6, 4, 8, 8, generator=torch.Generator().manual_seed(3))
    if seed_torch is not None:
        torch.manual_seed(seed_torch)
    return sampler(lambda inp, sigma, cc: 0.5 * inp + 0.1 * torch.tanh(inp), x, cond={}, uc={}, num_steps=steps)


@pytest.mark.parametrize("kind", ["euler_ancestral", "dpmpp2s_ancestral"])
def test_noise_seed_follows_torch_manual_seed(kind):
    with use_backend(SamplerEmulOps("cpu", exact=True)):
        s = make_sampler(kind, 4, guided=False)
        a, b = cheap_run(s, 11), cheap_run(s, 11)
        other = cheap_run(s, 12)
        fixed = cheap_run(make_sampler(kind, 4, guided=False, noise_seed=5))
        fixed2 = cheap_run(make_sampler(kind, 4, guided=False, noise_seed=5), 99)
    assert torch.equal(a, b)
    assert (a - other).abs().max() > 1e-2
    assert torch.equal(fixed, fixed2)                # an explicit noise_seed does not look at torch's generator
    assert (fixed - a).abs().max() > 1e-2


def test_user_noise_sampler_is_honoured():
    """noise_sampler is the reference's hook: a callable replaces the device generator (called once per step, like the reference)."""
    with use_backend(SamplerEmulOps("cpu", exact=True)):
        base = cheap_run(make_sampler("euler_ancestral", 4, guided=False, noise_seed=7))
        s = make_sampler("euler_ancestral", 4, guided=False, noise_seed=7)
        draws = []

        def same_numbers(x):                        # the device generator's numbers, through the hook
            draws.append(x.shape)
            return randn_ref(x.shape, 7, len(draws) - 1)

        s.noise_sampler = same_numbers
        via_hook = cheap_run(s)
        z = make_sampler("euler_ancestral", 4, guided=False, noise_seed=7)
        z.noise_sampler = torch.zeros_like
        no_noise = cheap_run(z)
        det = make_sampler("euler_ancestral", 4, guided=False, noise_seed=7)
        det.eta = 0.0                               # eta 0: plain Euler, no noise
        euler = cheap_run(det)
    assert len(draws) == 4
    assert (via_hook - base).abs().max() <= 1e-5
    assert (no_noise - base).abs().max() > 1e-2
    # zero noise leaves only the ancestral Euler steps to sigma_down: a deterministic path of its own
    assert torch.isfinite(no_noise).all() and (no_noise - euler).abs().max() > 1e-3


def test_reference_yaml_with_dpmpp2m(tmp_path):
    """A reference-format config naming sgm.modules.diffusionmodules.sampling.DPMPP2MSampler loads, instantiates and samples."""
    yaml = pytest.importorskip("yaml")
    from v3d_amd import configs
    from v3d_amd.sgm.util import instantiate_from_config
    ref = "sgm.modules.diffusionmodules."
    cfg = {"model": {"target": "sgm.models.diffusion.DiffusionEngine", "params": {"sampler_config": {
        "target": ref + "sampling.DPMPP2MSampler", "params": {
            "num_steps": 3, "verbose": False,
            "discretization_config": {"target": ref + "discretizer.EDMDiscretization", "params": {"sigma_max": 700.0}},
            "guider_config": {"target": ref + "guiders.LinearPredictionGuider", "params": {"max_scale": 2.5, "min_scale": 1.0, "num_frames": 3}}}}}}}
    path = tmp_path / "v3d.yaml"
    path.write_text(yaml.safe_dump(cfg))
    sc = configs.load_reference_yaml(str(path))["model"]["params"]["sampler_config"]
    assert sc["target"] == "v3d_amd.sgm.modules.diffusionmodules.sampling.DPMPP2MSampler"
    sc["params"]["device"] = "cpu"
    smp = instantiate_from_config(sc)
    assert isinstance(smp, sampling.DPMPP2MSampler)
    x = torch.randn(3, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    cond = {"crossattn": torch.zeros(3, 1, 8), "vector": torch.zeros(3, 8), "concat": torch.zeros(3, 4, 8, 8)}
    calls = [0]

    def den(inp, sigma, cc):
        calls[0] += 1
        return 0.3 * inp
    with use_backend(SamplerEmulOps("cpu", exact=True)):
        z = smp(den, x, cond=cond, uc=cond)
    assert calls[0] == 3 and torch.isfinite(z).all()


def test_v3d_512_config_sampler_choice():
    from v3d_amd import configs
    from v3d_amd.sgm.util import get_obj_from_str
    assert configs.v3d_512_config()["model"]["params"]["sampler_config"]["target"].endswith(".EulerEDMSampler")
    for name, cls in configs.SAMPLERS.items():
        target = configs.v3d_512_config(sampler=name)["model"]["params"]["sampler_config"]["target"]
        assert get_obj_from_str(target) is getattr(sampling, cls)
    with pytest.raises(ValueError):
        configs.v3d_512_config(sampler="ddim")


# The reference's signatures (sgm/modules/diffusionmodules/sampling.py), written down here: the tests do not read the reference checkout.
# (name, kind, default); kinds: P = positional-or-keyword, V = *args, K = **kwargs; `_` = no default
REF_INIT = {
    "AncestralSampler": [("eta", "P", 1.0), ("s_noise", "P", 1.0), ("args", "V", "_"), ("kwargs", "K", "_")],
    "EulerAncestralSampler": [("eta", "P", 1.0), ("s_noise", "P", 1.0), ("args", "V", "_"), ("kwargs", "K", "_")],
    "DPMPP2SAncestralSampler": [("eta", "P", 1.0), ("s_noise", "P", 1.0), ("args", "V", "_"), ("kwargs", "K", "_")],
    "LinearMultistepSampler": [("order", "P", 4), ("args", "V", "_"), ("kwargs", "K", "_")],
    "DPMPP2MSampler": [("discretization_config", "P", "_"), ("num_steps", "P", None), ("guider_config", "P", None), ("verbose", "P", False),
                       ("device", "P", "cuda")],
}
REF_CALL = {
    "AncestralSampler": ["denoiser", "x", "cond", "uc", "num_steps"],
    "EulerAncestralSampler": ["denoiser", "x", "cond", "uc", "num_steps"],
    "DPMPP2SAncestralSampler": ["denoiser", "x", "cond", "uc", "num_steps"],
    "LinearMultistepSampler": ["denoiser", "x", "cond", "uc", "num_steps", "kwargs"],
    "DPMPP2MSampler": ["denoiser", "x", "cond", "uc", "num_steps", "kwargs"],
}
REF_STEP = {
    "EulerAncestralSampler": ["sigma", "next_sigma", "denoiser", "x", "cond", "uc"],
    "DPMPP2SAncestralSampler": ["sigma", "next_sigma", "denoiser", "x", "cond", "uc", "kwargs"],
    "DPMPP2MSampler": ["old_denoised", "previous_sigma", "sigma", "next_sigma", "denoiser", "x", "cond", "uc"],
}
_KIND = {inspect.Parameter.POSITIONAL_OR_KEYWORD: "P", inspect.Parameter.VAR_POSITIONAL: "V", inspect.Parameter.VAR_KEYWORD: "K",
         inspect.Parameter.KEYWORD_ONLY: "KO"}


def _params(fn):
    return [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]


@pytest.mark.parametrize("name", list(REF_INIT))
def test_constructor_signatures_match_the_reference(name):
    """Same parameters in the same order with the same defaults; additions are keyword-only with a default (noise_seed)."""
    ps = _params(getattr(sampling, name).__init__)
    ours = [(p.name, _KIND[p.kind], "_" if p.default is inspect.Parameter.empty else p.default) for p in ps if _KIND[p.kind] != "KO"]
    assert ours == REF_INIT[name]
    for p in ps:
        if _KIND[p.kind] == "KO":
            assert p.default is not inspect.Parameter.empty, p.name


@pytest.mark.parametrize("name", list(REF_CALL))
def test_call_and_step_signatures_match_the_reference(name):
    cls = getattr(sampling, name)
    assert [p.name for p in _params(cls.__call__)] == REF_CALL[name]
    if name in REF_STEP:
        assert [p.name for p in _params(cls.sampler_step)] == REF_STEP[name]


def test_linear_multistep_coeff_against_quadrature():
    integrate = pytest.importorskip("scipy.integrate")
    t = [700.0, 60.0, 9.0, 1.5, 0.2, 0.0]

    def ref(order, i, j):
        def fn(tau):
            prod = 1.0
            for k in range(order):
                if j != k:
                    prod *= (tau - t[i - k]) / (t[i - j] - t[i - k])
            return prod
        return integrate.quad(fn, t[i], t[i + 1], epsrel=1e-10)[0]

    for i in range(len(t) - 1):
        order = min(i + 1, 4)
        for j in range(order):
            assert abs(linear_multistep_coeff(order, t, i, j) - ref(order, i, j)) <= 1e-9 * max(1.0, abs(ref(order, i, j)))
    with pytest.raises(ValueError):
        linear_multistep_coeff(3, t, 1, 0)


def test_ancestral_step_split():
    down, up = get_ancestral_step(10.0, 4.0, eta=1.0)
    assert abs(down ** 2 + up ** 2 - 16.0) < 1e-9 and 0 < up < 4.0
    assert get_ancestral_step(10.0, 4.0, eta=0.0) == (4.0, 0.0)
    assert get_ancestral_step(10.0, 0.0) == (0.0, 0.0)


def test_lms_order_beyond_one_kernel_call():
    """order 7 needs 8 terms in the update: applied in chunks of the 6-term kernel (x + 5 derivatives, then x + the rest), same result
    as a plain sum."""
    with use_backend(SamplerEmulOps("cpu", exact=True)):
        s = sampling.LinearMultistepSampler(7, discretization_config=disc_config(), num_steps=9, device="cpu")
        x = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(2))
        z = s(lambda inp, sigma, cc: 0.5 * inp, x.clone(), cond={}, uc={})
    # against a float64 restatement of the reference's loop (ds list, plain sum)
    sig =[float(v) for v in sampling.instantiate_from_config(disc_config())(9, device="cpu").float()]
    xr = x.double() * (1.0 + sig[0] ** 2) ** 0.5
    ds = []
    for i in range(9):
        ds.append((xr - 0.5 * xr) / sig[i])
        o = min(i + 1, 7)
        xr = xr + sum(linear_multistep_coeff(o, sig, i, j) * ds[-1 - j] for j in range(o))
    rel, cos = rel_cos(z, xr)
    assert rel <= 1e-4, rel
