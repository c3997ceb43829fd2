"""LoRA adapters without a GPU: the three naming schemes, alpha and scale arithmetic, the refusal of modules the layout does not have, the
order of clear / add calls the pipeline makes (stub model), the merge on the parameters in torch, and the four exports in the header."""
import os
import re

import pytest
import torch

from kit import ABI_VERSION_PIN, GOLDEN, ROOT  # noqa: E402


@pytest.fixture(scope="module")
def peft_sd():
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLDEN, "lora_tiny.safetensors"))


def as_diffusers(sd):
    return {k.replace("base_model.model.", "transformer."): v for k, v in sd.items()}


def as_peft_default(sd):
    return {k.replace(".lora_A.weight", ".lora_A.default.weight").replace(".lora_B.weight", ".lora_B.default.weight"): v for k, v in sd.items()}


def as_kohya(sd):
    out = {}
    for k, v in sd.items():
        stem, role = re.match(r"^base_model\.model\.(.+)\.(lora_A\.weight|lora_B\.weight|alpha)$", k).groups()
        role = {"lora_A.weight": "lora_down.weight", "lora_B.weight": "lora_up.weight", "alpha": "alpha"}[role]
        out[f"lora_unet_{stem.replace('.', '_')}.{role}"] = v
    return out


def test_three_naming_schemes_map_to_the_same_engine_keys(peft_sd, tiny_sd):
    from kandinsky.lora import load_lora
    ref = load_lora(peft_sd, known_keys=tiny_sd.keys())
    assert len(ref) == 22 and all(k.endswith(".weight") and k in tiny_sd for k in ref)
    for k, (A, B, alpha) in ref.items():
        assert (B.shape[0], A.shape[1]) == tuple(tiny_sd[k].shape) and A.shape[0] == B.shape[1]
    for name, conv in (("diffusers", as_diffusers), ("peft .default", as_peft_default), ("kohya", as_kohya)):
        got = load_lora(conv(peft_sd), known_keys=tiny_sd.keys())
        assert sorted(got) == sorted(ref), name
        for k in ref:
            assert torch.equal(got[k][0], ref[k][0]) and torch.equal(got[k][1], ref[k][1]) and got[k][2] == ref[k][2], (name, k)
    # from the file, without the model's keys: the layout alone decides
    assert sorted(load_lora(os.path.join(GOLDEN, "lora_tiny.safetensors"))) == sorted(ref)


def test_alpha_and_scale_arithmetic(peft_sd):
    from kandinsky.lora import load_lora, lora_scale
    ent = load_lora(peft_sd)
    with_alpha = {k: v for k, v in ent.items() if v[2] is not None}
    assert 0 < len(with_alpha) < len(ent)                      # the fixture holds both kinds
    for k, (A, B, alpha) in with_alpha.items():
        assert alpha == float(peft_sd[f"base_model.model.{k[:-7]}.alpha"])
        assert lora_scale(0.5, alpha, A.shape[0]) == 0.5 * alpha / A.shape[0]
    assert lora_scale(0.8, None, 16) == 0.8 and lora_scale(1.0, 8.0, 16) == 0.5 and lora_scale(2.0, 4.0, 4) == 2.0


def test_unknown_module_raises_keyerror_naming_it(tiny_sd):
    from kandinsky.lora import load_lora
    A, B = torch.zeros(2, 128), torch.zeros(128, 2)
    for bad in ("base_model.model.visual_transformer_blocks.0.self_attention.to_gate",
                "transformer.text_embeddings.norm", "base_model.model.vae.decoder.conv_in"):
        with pytest.raises(KeyError, match=re.escape(bad.split(".", 2)[2] if bad.startswith("base_model") else bad.split(".", 1)[1])):
            load_lora({bad + ".lora_A.weight": A, bad + ".lora_B.weight": B})
    with pytest.raises(KeyError, match="visual_transformer_blocks_0_self_attention_to_gate"):
        load_lora({"lora_unet_visual_transformer_blocks_0_self_attention_to_gate.lora_down.weight": A})
    ok = "base_model.model.visual_transformer_blocks.7.self_attention.to_query"      # in the layout, but this model has 2 visual blocks
    sd = {ok + ".lora_A.weight": A, ok + ".lora_B.weight": B}
    assert list(load_lora(sd)) == ["visual_transformer_blocks.7.self_attention.to_query.weight"]
    with pytest.raises(KeyError, match=r"visual_transformer_blocks\.7\.self_attention\.to_query"):
        load_lora(sd, known_keys=tiny_sd.keys())
    with pytest.raises(KeyError, match="lora_B"):
        load_lora({ok + ".lora_A.weight": A})


class StubDit:
    def __init__(self):
        self.calls = []

    def clear_lora(self):
        self.calls.append(("clear",))
        return self

    def add_lora(self, adapter, strength=1.0):
        self.calls.append(("add", adapter, strength))
        return self


def _pipe(dit):
    from types import SimpleNamespace as NS
    from kandinsky.t2v_pipeline import Kandinsky5T2VPipeline
    return Kandinsky5T2VPipeline("cpu", dit, None, None, conf=NS(model=NS(num_steps=4, guidance_weight=5.0)))


def test_set_lora_clears_then_adds_in_order():
    dit = StubDit()
    pipe = _pipe(dit)
    pipe.set_lora("a.safetensors", 0.5)
    assert dit.calls == [("clear",), ("add", "a.safetensors", 0.5)]
    dit.calls.clear()
    pipe.set_lora(["a", "b"], [0.25, 2.0])
    assert dit.calls == [("clear",), ("add", "a", 0.25), ("add", "b", 2.0)]
    dit.calls.clear()
    pipe.set_lora(["a", "b"], 0.75)                       # one strength for all
    assert dit.calls == [("clear",), ("add", "a", 0.75), ("add", "b", 0.75)]
    dit.calls.clear()
    pipe.set_lora(None)
    assert dit.calls == [("clear",)]
    with pytest.raises(ValueError, match="2 LoRA adapter"):
        pipe.set_lora(["a", "b"], [1.0, 2.0, 3.0])


def test_get_pipeline_lora_keyword(monkeypatch, tmp_path):
    import kandinsky.utils as U
    import kandinsky.models.text_embedders as TE
    import kandinsky.models.vae as V
    import safetensors.torch as ST
    import yaml
    from kandinsky.config import default_configs

    class Stub(StubDit):
        def to(self, *a, **k):
            return self

        def eval(self):
            return self

        def load_state_dict(self, *a, **k):
            self.calls.append(("load",))

    dits = []
    monkeypatch.setattr(TE, "get_text_embedder", lambda conf: Stub())
    monkeypatch.setattr(V, "build_vae", lambda conf: Stub())
    monkeypatch.setattr(U, "get_dit", lambda params: dits.append(Stub()) or dits[-1])
    monkeypatch.setattr(ST, "load_file", lambda path: {})
    path = tmp_path / "config_5s_sft.yaml"
    path.write_text(yaml.safe_dump(default_configs()["config_5s_sft.yaml"], sort_keys=False))
    pipe = U.get_T2V_pipeline("cpu", conf_path=str(path))
    assert dits[-1].calls == [("load",)]                   # no adapter: the model is not touched
    pipe = U.get_T2V_pipeline("cpu", conf_path=str(path), lora=["x.safetensors", "y.safetensors"], lora_scale=[0.5, 1.5])
    assert dits[-1].calls == [("load",), ("clear",), ("add", "x.safetensors", 0.5), ("add", "y.safetensors", 1.5)]   # after the weights
    pipe.set_lora("z.safetensors")
    assert dits[-1].calls[-2:] == [("clear",), ("add", "z.safetensors", 1.0)]


def test_cli_lora_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("k5_cli_lora", os.path.join(ROOT, "kandinsky-5_amd", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.build_parser().parse_args(["--lora", "a.safetensors", "--lora", "b.safetensors", "--lora_scale", "0.5", "2"])
    assert a.lora == ["a.safetensors", "b.safetensors"] and a.lora_scale == [0.5, 2.0]
    a = cli.build_parser().parse_args([])
    assert getattr(a, "lora", None) is None and getattr(a, "lora_scale", 1.0) == 1.0


def test_torch_path_merge_equals_fp32_formula_and_clear_restores(peft_sd, tiny_sd, golden_meta):
    """No engine built: add_lora merges on the parameters in torch, W + s * B @ A in fp32; clear_lora puts the loaded values back."""
    from kandinsky.lora import load_lora, lora_scale, merge_torch
    from kandinsky.models.dit import DiffusionTransformer3D
    dit = DiffusionTransformer3D(**golden_meta["tiny_config"])
    dit.load_state_dict({k: v.clone() for k, v in tiny_sd.items()}, assign=True)
    ent = load_lora(peft_sd, known_keys=tiny_sd.keys())
    dit.add_lora(peft_sd, strength=0.75)
    sd = dit.state_dict()
    for k, v in tiny_sd.items():
        if k in ent:
            A, B, alpha = ent[k]
            want = v.float() + lora_scale(0.75, alpha, A.shape[0]) * (B.float() @ A.float())
            assert torch.equal(sd[k], want.to(v.dtype)), k
            assert not torch.equal(sd[k], v), k
        else:
            assert torch.equal(sd[k], v), k
    st = dit.lora_state()
    assert st["matrices"] == len(ent) and st["backup_bytes"] == sum(tiny_sd[k].numel() * tiny_sd[k].element_size() for k in ent)
    dit.add_lora(peft_sd, strength=-0.25)                 # a second one merges onto the first; the saved copies stay the loaded values
    dit.clear_lora()
    assert all(torch.equal(dit.state_dict()[k], v) for k, v in tiny_sd.items())
    assert dit.lora_state() == {"adapters": 0, "matrices": 0, "backup_bytes": 0}
    W = torch.randn(5, 7).bfloat16()
    A, B = torch.randn(3, 7).half(), torch.randn(5, 3)
    assert torch.equal(merge_torch(W, A, B, -0.5), (W.float() - 0.5 * (B.float() @ A.float())).bfloat16())
    bad = {"base_model.model.time_embeddings.in_layer.lora_A.weight": torch.zeros(2, 5), "base_model.model.time_embeddings.in_layer.lora_B.weight": torch.zeros(64, 2)}
    with pytest.raises(ValueError, match="do not fit"):
        dit.add_lora(bad)


def test_header_declares_the_four_exports_under_the_same_abi():
    src = open(os.path.join(ROOT, "include", "k5.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("k5_lora_merge", "k5_dit_add_lora", "k5_dit_clear_lora", "k5_dit_lora_state"):
        assert re.search(rf"\bint {name}\s*\(", code), name
    assert "#define K5_ABI_VERSION %d" % ABI_VERSION_PIN in src
    from kandinsky import _engine as E
    assert {"k5_lora_merge", "k5_dit_add_lora", "k5_dit_clear_lora", "k5_dit_lora_state"} <= set(E.SYMBOLS)
