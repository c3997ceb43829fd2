"""The scaffolding that the sampler and kernel suites share: paths and constants, the error measures, the tiny model and its wrapper, the
golden prompts, one generate() call for the GPU suites and one for the host suites, the module-scoped fixtures, and the header/binding/library
agreement check.  A plain module, imported by name; a file binds its own shape, step count and positions once (functools.partial or a
two-line def) and its call sites read as before."""
import ctypes as C
import os
import re
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kandinsky-5_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
K5_ERR_ARG, K5_ERR_ALIGN, K5_ERR_STATE, K5_ERR_UNSUPPORTED = 1, 2, 4, 6   # include/k5.h
ABI_VERSION_PIN = 11
BF = torch.bfloat16
SHAPE = (3, 8, 12, 16)                                          # the golden latent: 72 tokens
POS = [torch.arange(3), torch.arange(4), torch.arange(6)]       # its rope positions


def flash_conf():
    return NS(model=NS(dit_params=NS(patch_size=(1, 2, 2)), attention=NS(type="flash")), metrics=NS(scale_factor=(1.0, 2.0, 2.0)))


# ------------------------------------------------------------------------------------------ numerics
def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def f32(x):
    return float(np.float32(x))


def bfr(x):
    return x.to(BF).float()


# ------------------------------------------------------------------------------------------ the tiny model
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")


def tiny_config(golden_meta):
    c = dict(golden_meta["tiny_config"])
    c["patch_size"], c["axes_dims"] = tuple(c["patch_size"]), tuple(c["axes_dims"])
    return c


def make_dit(cfg, sd, *, engine=False, **over):
    """the model on the GPU, its constructor arguments overridden by `over`; engine=True builds its engine at once"""
    from kandinsky.models.dit import DiffusionTransformer3D
    d = DiffusionTransformer3D(**dict(cfg, **over))
    d.load_state_dict(sd, assign=True)
    d = d.to("cuda:0")
    if engine:
        d.engine("cuda:0")
    return d


def host_tiny(golden_meta):
    from kandinsky.models.dit import DiffusionTransformer3D
    return DiffusionTransformer3D(**tiny_config(golden_meta))


class Wrapped(torch.nn.Module):
    """Any non-DiffusionTransformer3D callable takes the per-step path of generate.  That path looks at the wrapper's attributes, so nothing
    is handed on unasked: `blocks` hands num_visual_blocks on, `hand_on` names the model's methods and settings to hand on (forward_skip, a
    setting's set_/clear_ pair and its state), and `refuse` makes every forward fail the test, for calls that must be refused first."""
    def __init__(self, m, *, blocks=False, hand_on=(), refuse=False):
        super().__init__()
        self.m, self.visual_cond, self.hand_on, self.refuse = m, m.visual_cond, tuple(hand_on), refuse
        if blocks:
            self.num_visual_blocks = m.num_visual_blocks

    def forward(self, *a, **k):
        if self.refuse:
            pytest.fail("refused calls must not run the model")
        return self.m(*a, **k)

    def __getattr__(self, name):
        if name in self.__dict__.get("hand_on", ()):
            return self.forward if self.refuse else getattr(self.m, name)
        return super().__getattr__(name)


# ------------------------------------------------------------------------------------------ inputs
def prompts(golden):
    te = {"text_embeds": golden["fwd.text"].cuda(), "pooled_embed": golden["fwd.pooled"].cuda()}
    ne = {"text_embeds": golden["gen.null_text"].cuda(), "pooled_embed": golden["gen.null_pooled"].cuda()}
    return te, ne


def host_prompt(n, seed=0, *, dims):
    g = torch.Generator().manual_seed(seed)
    return {"text_embeds": torch.randn(n, dims[0], generator=g), "pooled_embed": torch.randn(1, dims[1], generator=g)}


def edit_mask(shape=SHAPE):
    """frame 0 and the left half of the other frames kept, then a band of 0.25, the rest free"""
    T, H, W, _ = shape
    m = torch.zeros(T, H, W, 1)
    m[0] = 1.0
    m[1:, :, :W // 2] = 1.0
    m[1:, :, W // 2:W // 2 + 2] = 0.25
    return m


def source_latent(shape=SHAPE, seed=77):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rank_case():
    g = torch.Generator().manual_seed(5)
    shape = (8, 16, 16, 16)
    noise = torch.randn(*shape, generator=g)
    te = {"text_embeds": torch.randn(9, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    ne = {"text_embeds": torch.randn(4, 96, generator=g).cuda(), "pooled_embed": torch.randn(1, 48, generator=g).cuda()}
    return shape, noise, te, ne


def _sp_case():
    """the rank workers' edit case with its prompts on the GPU: shape, noise, te, ne, source latent, keep mask"""
    from edit_rank_worker import case
    shape, noise, te, ne, src, mask = case()
    return shape, noise, {k: v.cuda() for k, v in te.items()}, {k: v.cuda() for k, v in ne.items()}, src, mask


# ------------------------------------------------------------------------------------------ generate()
def run_generate(model, golden, w, *, steps, shape, pos, noise=None, te=None, text_pos=None, **kw):
    """generate() on the GPU from the golden prompts and, unless given, the golden noise"""
    from kandinsky.generation_utils import generate
    base, ne = prompts(golden)
    noise = golden["gen.noise"] if noise is None else noise
    return generate(model, "cuda:0", shape, steps, base if te is None else te, ne, pos, torch.arange(7) if text_pos is None else text_pos,
                    torch.arange(4), w, 5.0, flash_conf(), noise=noise, **kw)


def call_generate(model, *, w, steps, shape, pos, conf, prompt, **kw):
    """generate() on the CPU from zero noise and the prompts prompt(7), prompt(4, 1): for the refusals and the host-side plans"""
    from kandinsky.generation_utils import generate
    return generate(model, "cpu", shape, steps, prompt(7), prompt(4, 1), pos, torch.arange(7), torch.arange(4), w, 5.0, conf,
                    noise=torch.zeros(shape), **kw)


# ------------------------------------------------------------------------------------------ fixtures, one instance per importing module
@pytest.fixture(scope="module")
def cfg(golden_meta):
    return tiny_config(golden_meta)


@pytest.fixture(scope="module")
def tiny_dit(cfg, tiny_sd):
    need_gpu()
    return make_dit(cfg, tiny_sd)


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, PKG)
    import build as k5build
    return k5build.build(verbose=False)


@pytest.fixture(scope="module")
def E():
    need_gpu()
    from kandinsky import _engine
    _engine.lib()
    return _engine


# ------------------------------------------------------------------------------------------ header, binding and library
def assert_abi_entries(built_lib, names, structs=()):
    """The header, the ctypes binding and the built library agree: on the pinned ABI version, on every entry in `names` (declared outside
    comments, bound, exported, with as many arguments as the binding gives), and on every (struct name, ctypes class) in `structs`, which
    has the header's fields in the header's order."""
    from kandinsky import _engine as E
    hdr = open(os.path.join(ROOT, "include", "k5.h")).read()
    assert int(re.search(r"#define K5_ABI_VERSION (\d+)", hdr).group(1)) == ABI_VERSION_PIN == E.ABI_VERSION
    lib = C.CDLL(built_lib)
    assert lib.k5_abi_version() == ABI_VERSION_PIN
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in names:
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, code, flags=re.S)
        assert decl, name
        assert name in E.SYMBOLS and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(E.SYMBOLS[name][1]), name
    for struct, binding in structs:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        fields = [re.search(r"(\w+)\s*$", decl.strip()).group(1) for decl in body.replace(",", ";").split(";") if decl.strip()]
        assert fields == [f[0] for f in binding._fields_], struct
