"""LoRA on the 2B layout: what `add_lora` over every linear layer costs against the only route without it.

    python tools/lora_bench.py [--rank 64] [--out profiles/lora_bench.json]

Model: the LITE 2B layout (model_dim 1792, ff_dim 7168, 2 text + 32 visual blocks) on synthetic weights (init_synthetic, drawn on the
device).  The adapter: every rank-2 weight of the state dict, rank R, bf16 factors already on the device.
  merge    one `add_lora` over all of them (k5_dit_add_lora per key: backup copy + merge kernel + device synchronise), then `clear_lora`
  rebuild  what a handle without the feature has to do: destroy, create, load the (host-merged) weights again, finalize — here with the
           weights already on the device, so the upload of a host checkpoint is NOT in the figure (it would add its bytes over PCIe)
Wall-clock seconds around synchronised calls; the traffic floor is one read and one write of the touched weights (plus the backup's
read and write on the first merge)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kandinsky-5_amd"))
import torch  # noqa: E402

LITE = dict(in_visual_dim=16, out_visual_dim=16, time_dim=512, patch_size=(1, 2, 2), model_dim=1792, ff_dim=7168, num_text_blocks=2,
            num_visual_blocks=32, axes_dims=(16, 24, 24), visual_cond=True, in_text_dim=3584, in_text_dim2=768)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kandinsky.models.dit import DiffusionTransformer3D
    dev = torch.device("cuda:0")
    with torch.device("meta"):
        dit = DiffusionTransformer3D(**LITE)
    dit.init_synthetic(dev, seed=0)
    shapes = {k: tuple(v.shape) for k, v in dit.state_dict().items() if v.dim() == 2}
    g = torch.Generator(device=dev).manual_seed(1)
    R = a.rank
    entries = {k: ((torch.randn(R, c, device=dev, generator=g) * 0.02).bfloat16(), (torch.randn(r, R, device=dev, generator=g) * 0.02).bfloat16(), None)
               for k, (r, c) in shapes.items()}
    params = sum(r * c for r, c in shapes.values())
    packed_bytes = sum(r * c * (4 if ("time_embeddings." in k or "modulation.out_layer." in k) else 2) for k, (r, c) in shapes.items())
    flop = 2.0 * R * params
    torch.cuda.synchronize()
    merge_s, clear_s, second_s = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter(); dit._engine_add_lora(entries, 1.0); torch.cuda.synchronize(); merge_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); dit._engine_add_lora(entries, 0.5); torch.cuda.synchronize(); second_s.append(time.perf_counter() - t0)   # backups exist
        dit._lora = [(entries, 1.0)]
        t0 = time.perf_counter(); dit.clear_lora(); torch.cuda.synchronize(); clear_s.append(time.perf_counter() - t0)
    state = dit.lora_state()
    rebuild_s = []
    for i in range(a.repeats):
        t0 = time.perf_counter(); dit.init_synthetic(dev, seed=1 + i); torch.cuda.synchronize(); rebuild_s.append(time.perf_counter() - t0)
    res = {"layout": "LITE 2B, 2 + 32 blocks", "rank": R, "matrices": len(shapes), "params_touched": params, "packed_bytes": packed_bytes,
           "merge_tflop": flop / 1e12,
           "add_lora_first_s": min(merge_s), "add_lora_again_s": min(second_s), "clear_lora_s": min(clear_s),
           "rebuild_device_weights_s": min(rebuild_s),
           "add_lora_again_effective_GBps": 2 * packed_bytes / min(second_s) / 1e9, "add_lora_again_TFLOPs": flop / min(second_s) / 1e12,
           "all": {"add_first": merge_s, "add_again": second_s, "clear": clear_s, "rebuild": rebuild_s}, "state_after_clear": state}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
