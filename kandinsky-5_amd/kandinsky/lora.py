"""LoRA adapters for the DiT: read an adapter file, map its module names onto the engine's state_dict keys, work out the scale.

The reference has no adapter code; front ends merge `W + scale * (B @ A)` on the host before `load_state_dict`.  Here the merge runs inside
the engine on the packed weights (`k5_dit_add_lora`, include/k5.h) and is undone by `k5_dit_clear_lora`, so changing an adapter or its
strength costs one pass over the touched matrices instead of a 4 GB upload and a re-pack.

Accepted naming schemes, all for rank-2 linear weights of the DiT only (no DoRA / LoCon, no text encoders, no VAE):
    peft       base_model.model.<module>.lora_A[.default].weight / lora_B[.default].weight
    diffusers  transformer.<module>.lora_A.weight / lora_B.weight
    kohya      lora_unet_<module with _ for .>.lora_down.weight / lora_up.weight / .alpha
`<module>.alpha` (a scalar) is honoured in the first two schemes as well.  lora_A / lora_down is A [R][in], lora_B / lora_up is B [out][R].
"""
from __future__ import annotations

import re
from typing import Dict, Iterable, Optional, Tuple

import torch

# linear modules of the checkpoint layout, dotted
_TOP = ("time_embeddings.in_layer", "time_embeddings.out_layer", "text_embeddings.in_layer", "pooled_text_embeddings.in_layer",
        "visual_embeddings.in_layer", "out_layer.modulation.out_layer", "out_layer.out_layer")
_ATTN = ("to_query", "to_key", "to_value", "out_layer")
_FF = ("feed_forward.in_layer", "feed_forward.out_layer")
_TEXT_BLOCK = ("text_modulation.out_layer",) + tuple(f"self_attention.{n}" for n in _ATTN) + _FF
_VISUAL_BLOCK = (("visual_modulation.out_layer",) + tuple(f"self_attention.{n}" for n in _ATTN)
                 + tuple(f"cross_attention.{n}" for n in _ATTN) + _FF)
_BLOCKS = {"text_transformer_blocks": _TEXT_BLOCK, "visual_transformer_blocks": _VISUAL_BLOCK}

_PREFIXES = ("base_model.model.", "transformer.", "diffusion_model.", "model.")
_DOWN = ("lora_A.default.weight", "lora_A.weight", "lora_down.weight")
_UP = ("lora_B.default.weight", "lora_B.weight", "lora_up.weight")


def resolve_module(name: str, sep: str = ".") -> str:
    """The dotted module name of the checkpoint layout for `name` written with `sep` between its parts ('.' or, kohya, '_').
    KeyError naming the module when the layout has no such linear layer."""
    for m in _TOP:
        if name == m.replace(".", sep):
            return m
    for blocks, subs in _BLOCKS.items():
        m = re.match(rf"^{blocks}{re.escape(sep)}(\d+){re.escape(sep)}(.+)$", name)
        if m:
            for sub in subs:
                if m.group(2) == sub.replace(".", sep):
                    return f"{blocks}.{int(m.group(1))}.{sub}"
    raise KeyError(f"LoRA module {name!r} is not a linear layer of the Kandinsky-5 DiT checkpoint layout")


def _split(key: str) -> Optional[Tuple[str, str, str]]:
    """adapter tensor name -> (module as written, separator, role) with role in 'A' / 'B' / 'alpha'; None = not an adapter tensor"""
    role = None
    for suffixes, r in ((_DOWN, "A"), (_UP, "B"), (("alpha",), "alpha")):
        for suf in suffixes:
            if key.endswith("." + suf):
                role, stem = r, key[: -len(suf) - 1]
                break
        if role:
            break
    if role is None:
        return None
    if stem.startswith("lora_unet_"):
        return stem[len("lora_unet_"):], "_", role
    for p in _PREFIXES:
        if stem.startswith(p):
            stem = stem[len(p):]
            break
    return stem, ".", role


def load_lora(source, known_keys: Optional[Iterable[str]] = None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor, Optional[float]]]:
    """`source`: the path of a .safetensors file or a state dict of adapter tensors.  Returns {engine key: (A [R][in], B [out][R], alpha or
    None)}, the engine key being the state_dict key of the weight the adapter applies to (`<module>.weight`).  `known_keys` (the model's
    state_dict keys) additionally rejects a block index the model does not have.  A module outside the layout raises KeyError naming it."""
    if isinstance(source, dict):
        sd = source
    else:
        from safetensors.torch import load_file
        sd = load_file(str(source))
    known = None if known_keys is None else set(known_keys)
    parts: Dict[str, dict] = {}
    for key, t in sd.items():
        sp = _split(key)
        if sp is None:
            raise KeyError(f"{key!r} is not a LoRA tensor name (lora_A / lora_B / lora_down / lora_up / alpha expected)")
        written, sep, role = sp
        module = resolve_module(written, sep)
        engine_key = module + ".weight"
        if known is not None and engine_key not in known:
            raise KeyError(f"LoRA module {module!r}: the model has no {engine_key}")
        parts.setdefault(engine_key, {})[role] = t
    out = {}
    for engine_key, p in parts.items():
        if "A" not in p or "B" not in p:
            raise KeyError(f"LoRA adapter for {engine_key[:-7]!r} lacks its {'lora_A / lora_down' if 'A' not in p else 'lora_B / lora_up'} tensor")
        A, B = p["A"], p["B"]
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[1]:
            raise ValueError(f"LoRA adapter for {engine_key[:-7]!r}: A {tuple(A.shape)} and B {tuple(B.shape)} are not [R][in] and [out][R]")
        alpha = p.get("alpha")
        out[engine_key] = (A, B, None if alpha is None else float(torch.as_tensor(alpha).reshape(-1)[0]))
    return out


def lora_scale(strength: float, alpha: Optional[float], rank: int) -> float:
    """What the engine is given: strength * alpha / R, or strength when the adapter carries no alpha."""
    return float(strength) if alpha is None else float(strength) * float(alpha) / int(rank)


def merge_torch(W: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scale: float) -> torch.Tensor:
    """W + scale * (B @ A) in fp32, returned in W's dtype: the merge on a model whose engine is not built yet."""
    return (W.float() + float(scale) * (B.to(W.device).float() @ A.to(W.device).float())).to(W.dtype)


def as_list(lora, lora_scale_):
    """(paths, strengths) of the `lora=` / `lora_scale=` keywords: one or several adapters, one strength for all or one each."""
    if lora is None:
        return [], []
    loras = list(lora) if isinstance(lora, (list, tuple)) else [lora]
    scales = list(lora_scale_) if isinstance(lora_scale_, (list, tuple)) else [lora_scale_] * len(loras)
    if len(scales) == 1 and len(loras) > 1:
        scales = scales * len(loras)
    if len(scales) != len(loras):
        raise ValueError(f"{len(loras)} LoRA adapter(s) but {len(scales)} scale(s)")
    return loras, [float(s) for s in scales]
