"""The settings on the engine handle (watch, NAG, regions, guidance plan, skip set) on the MI355X, where the host test's recorder cannot
reach: that all of them together survive a rebuild of the engine bit for bit, and that an install the library refuses leaves the previous
setting installed and the memory the engine borrows for it alive."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from kit import K5_ERR_ARG, POS, make_dit, need_gpu, prompts, tiny_config  # noqa: E402


@pytest.fixture
def dit(golden_meta, tiny_sd):
    """a tiny model of its own per test: both tests leave the handle in a state of their making"""
    need_gpu()
    return make_dit(tiny_config(golden_meta), tiny_sd)


def other_prompt(n, seed):
    return {"text_embeds": torch.randn(n, 96, generator=torch.Generator().manual_seed(seed)).cuda()}


def forward(model, golden):
    te, _ = prompts(golden)
    return model(golden["fwd.x"].cuda(), te["text_embeds"], te["pooled_embed"], golden["fwd.time"], POS, torch.arange(7), scale_factor=(1.0, 2.0, 2.0))


def test_every_setting_survives_a_rebuild(dit, golden):
    """all five at once (the sampler accepts them together on a single-rank handle), installed on the live handle; after _destroy_engine
    the next call rebuilds the engine and re-installs them from the stored values: the same bits, every state on, the callback runs again"""
    from kandinsky.generation_utils import sigma_schedule
    te, ne = prompts(golden)
    dit.engine("cuda:0")
    steps = []
    dit.set_watch(lambda info: steps.append(info.step))                 # no previews
    dit.set_nag(ne, torch.arange(4), 5.0, 2.5, 0.25)
    half = torch.zeros(1, 3, 8, 12)
    half[..., :6] = 1.0
    dit.set_regions([other_prompt(5, 31)], [torch.arange(5)], half, 0.0)
    dit.set_guidance([5.0, 3.0, 4.0], False, 0, 0.7)
    dit.set_skip_guidance([1], 2.0)
    sigmas = sigma_schedule(3, 5.0).tolist()

    def run():
        latent = golden["gen.noise"].cuda().float().contiguous().clone()
        dit.sample(latent, sigmas, te, ne, POS, torch.arange(7), torch.arange(4), 5.0, scale_factor=(1.0, 2.0, 2.0))
        return latent

    def states():
        return [dit.watch_state()[0], dit.nag_state()[0], dit.regions_state()[0], dit.guidance_state()[0], dit.skip_state()[0]]

    first = run()
    assert steps == [0, 1, 2] and states() == [3, True, True, True, True]
    assert torch.isfinite(first).all() and not torch.equal(first, golden["gen.noise"].cuda())
    counts = dit.nag_state()[1], dit.regions_state()[2], dit.guidance_state()[1:], dit.skip_state()[1:]
    dit._destroy_engine()
    assert dit._handle is None and states() == [0, False, False, False, False]
    second = run()
    assert dit._handle is not None and torch.equal(first, second)
    assert steps == [0, 1, 2, 0, 1, 2] and states() == [3, True, True, True, True]
    assert (dit.nag_state()[1], dit.regions_state()[2], dit.guidance_state()[1:], dit.skip_state()[1:]) == counts   # the new handle did the same work
    assert counts[0] > 0 and counts[1] > 0 and counts[2] == (3, 0, 0) and counts[3][0] == 3


def test_a_refused_install_keeps_the_previous_setting_alive(dit, golden, monkeypatch):
    """the library (a proxy in front of it: the engine is not called) answers K5_ERR_ARG to one k5_dit_set_nag; the engine setters check
    before they write, so the handle still holds the first negative prompt and reads its tensors at the next forward"""
    from kandinsky import _engine as E
    _, ne = prompts(golden)
    plain = forward(dit, golden)
    dit.set_nag(ne, torch.arange(4), 5.0, 2.5, 0.25)
    guided = forward(dit, golden)
    assert not torch.equal(guided, plain)
    real = E.lib()

    class RefuseOnce:
        refused = 0

        def __getattr__(self, name):
            if name == "k5_dit_set_nag" and not self.refused:
                self.refused = 1
                return lambda *a: K5_ERR_ARG
            return getattr(real, name)

    proxy = RefuseOnce()
    monkeypatch.setattr(E, "lib", lambda: proxy)
    with pytest.raises(RuntimeError, match="k5_dit_set_nag"):
        dit.set_nag(other_prompt(6, 32), torch.arange(6), 3.0, 2.0, 1.0)
    assert proxy.refused == 1
    monkeypatch.undo()
    del ne
    gc.collect()                                                         # whatever the refused call dropped is gone now
    filler = [torch.full((4, 96), 7.0, device="cuda") for _ in range(8)]  # ... and its memory taken
    assert dit.nag_state()[0] is True and dit._nag["args"] == (5.0, 2.5, 0.25)
    assert torch.equal(forward(dit, golden), guided)
    dit.clear_nag()
    assert dit.nag_state()[0] is False and torch.equal(forward(dit, golden), plain)
    del filler
