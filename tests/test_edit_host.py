"""Host side of video-to-video / masked editing: the pixel keep mask pooled to the latent grid, per-frame preprocessing, the strength ->
first-step rule, reading clips back, and every refusal that needs no GPU."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from kandinsky.conditioning import encode_video, pixel_mask_to_latent, preprocess_image, preprocess_video
from kandinsky.generation_utils import edit_first_step, generate, generate_sample
from kandinsky.video_io import read_video, write_video


# ------------------------------------------------------------------------------------------ keep mask
def test_one_pixel_off_clears_exactly_its_cell():
    T, H, W = 3, 32, 48
    m = torch.ones(4 * (T - 1) + 1, H, W)
    m[6, 19, 41] = 0.0                                   # pixel frame 6 -> latent frame 2 (frames 5..8); cell (19 // 8, 41 // 8)
    lat = pixel_mask_to_latent(m, T, H, W)
    assert lat.shape == (T, H // 8, W // 8, 1) and lat.dtype == torch.float32
    want = torch.ones(T, H // 8, W // 8, 1)
    want[2, 2, 5] = 0.0
    assert torch.equal(lat, want)
    m[6, 19, 41] = 0.49                                  # below the threshold is off, at it is on
    assert torch.equal(pixel_mask_to_latent(m, T, H, W), want)
    m[6, 19, 41] = 0.5
    assert pixel_mask_to_latent(m, T, H, W).eq(1).all()


@pytest.mark.parametrize("frame,latent_frame", [(0, 0), (1, 1), (4, 1), (5, 2), (8, 2), (9, 3), (12, 3)])
def test_frame_zero_stands_alone_then_groups_of_four(frame, latent_frame):
    T, H, W = 4, 8, 16
    m = torch.ones(13, H, W, dtype=torch.bool)
    m[frame] = False
    lat = pixel_mask_to_latent(m, T, H, W)[..., 0]
    for t in range(T):
        assert lat[t].eq(0.0 if t == latent_frame else 1.0).all(), (t, lat[t])


def test_hw_mask_broadcasts_and_longer_masks_are_cut():
    T, H, W = 3, 16, 24
    m = torch.zeros(H, W)
    m[:, :12] = 1.0                                      # 1.5 cells wide: the half-covered column of cells is not kept
    lat = pixel_mask_to_latent(m, T, H, W)
    want = torch.zeros(T, 2, 3, 1)
    want[:, :, 0] = 1.0
    assert torch.equal(lat, want)
    assert torch.equal(pixel_mask_to_latent(m[None].expand(9, -1, -1), T, H, W), want)
    assert torch.equal(pixel_mask_to_latent(m[None].expand(20, -1, -1).numpy(), T, H, W), want)   # frames past 4(T-1)+1 ignored


def test_mask_refusals():
    with pytest.raises(ValueError, match="pixel frames"):
        pixel_mask_to_latent(torch.ones(8, 16, 24), 3, 16, 24)
    with pytest.raises(ValueError, match="mask must be"):
        pixel_mask_to_latent(torch.ones(16, 25), 3, 16, 24)
    with pytest.raises(ValueError, match="multiples of 8"):
        pixel_mask_to_latent(torch.ones(12, 24), 3, 12, 24)


# ------------------------------------------------------------------------------------------ frames
def test_preprocess_video_is_preprocess_image_per_frame():
    g = torch.Generator().manual_seed(3)
    clip = torch.randint(0, 256, (5, 30, 44, 3), generator=g, dtype=torch.uint8)
    out = preprocess_video(clip, 16, 24)
    assert out.shape == (5, 3, 16, 24) and out.dtype == torch.float32
    for f in range(5):
        assert torch.equal(out[f], preprocess_image(clip[f], 16, 24))
    fl = clip.permute(0, 3, 1, 2).float() / 127.5 - 1.0
    assert torch.equal(preprocess_video(fl, 16, 24), out)               # the float twin of a uint8 clip
    assert torch.equal(preprocess_video(clip.numpy(), 16, 24), out)
    for bad in (clip[0], clip.permute(0, 3, 1, 2), fl.permute(0, 2, 3, 1), clip[:0], clip.to(torch.int32)):
        with pytest.raises(ValueError):
            preprocess_video(bad, 16, 24)


def test_encode_video_takes_the_first_frames_and_refuses_a_short_clip():
    seen = {}

    class Vae:
        config = NS(scaling_factor=0.5)

        def encode(self, x):
            seen["x"] = x
            B, _, F, H, W = x.shape
            mean = torch.arange(B * 4 * ((F - 1) // 4 + 1) * (H // 8) * (W // 8), dtype=torch.float32).reshape(B, 4, (F - 1) // 4 + 1, H // 8, W // 8)
            return NS(latent_dist=NS(mean=mean))

    g = torch.Generator().manual_seed(5)
    clip = torch.randint(0, 256, (12, 16, 24, 3), generator=g, dtype=torch.uint8)
    z = encode_video(clip, Vae(), 3, 16, 24, vae_device="cpu")
    assert z.shape == (3, 2, 3, 4) and z.dtype == torch.float32 and z.is_contiguous()
    assert seen["x"].shape == (1, 3, 9, 16, 24)
    assert torch.equal(seen["x"][0].permute(1, 0, 2, 3), preprocess_video(clip[:9], 16, 24))
    assert torch.equal(z, (torch.arange(72, dtype=torch.float32).reshape(4, 3, 2, 3) * 0.5).permute(1, 2, 3, 0))
    with pytest.raises(ValueError, match="9 pixel frames"):
        encode_video(clip[:8], Vae(), 3, 16, 24, vae_device="cpu")
    with pytest.raises(ValueError, match="multiples of 8"):
        encode_video(clip, Vae(), 3, 12, 24, vae_device="cpu")


# ------------------------------------------------------------------------------------------ strength
@pytest.mark.parametrize("num_steps,strength,first", [
    (1, 0.01, 0), (1, 0.5, 0), (1, 1.0, 0),
    (4, 0.01, 3), (4, 0.3, 3), (4, 0.5, 2), (4, 0.75, 1), (4, 0.9, 0), (4, 1.0, 0),
    (25, 0.01, 24), (25, 0.5, 12), (25, 0.7, 7), (25, 1.0, 0),          # 12.5 + 0.5 = 13 steps run
    (50, 0.01, 49), (50, 0.5, 25), (50, 0.99, 0), (50, 1.0, 0)])
def test_strength_to_first_step(num_steps, strength, first):
    assert edit_first_step(num_steps, strength) == first


@pytest.mark.parametrize("strength", [0.0, -0.1, 1.0001, 2, float("nan")])
def test_strength_outside_the_unit_interval(strength):
    with pytest.raises(ValueError, match="strength"):
        edit_first_step(10, strength)


# ------------------------------------------------------------------------------------------ clips on disk
def test_read_video_round_trips_write_video(tmp_path):
    g = torch.Generator().manual_seed(1)
    clip = torch.randint(0, 256, (5, 16, 24, 3), generator=g, dtype=torch.uint8)
    written = write_video(str(tmp_path / "clip.mp4"), clip, fps=12)
    back = read_video(written)
    assert back.dtype == torch.uint8 and torch.equal(back, clip)


def test_read_video_npy_pt_and_directory(tmp_path):
    from PIL import Image
    g = torch.Generator().manual_seed(2)
    clip = torch.randint(0, 256, (4, 8, 16, 3), generator=g, dtype=torch.uint8)
    np.save(tmp_path / "clip.npy", clip.numpy())
    torch.save(clip, tmp_path / "clip.pt")
    assert torch.equal(read_video(str(tmp_path / "clip.npy")), clip)
    assert torch.equal(read_video(str(tmp_path / "clip.pt")), clip)
    d = tmp_path / "frames"
    d.mkdir()
    for i in (2, 0, 3, 1):                               # written out of order: name order decides
        Image.fromarray(clip[i].numpy()).save(d / f"f_{i:03d}.png")
    (d / "notes.txt").write_text("not a frame")
    assert torch.equal(read_video(str(d)), clip)
    np.save(tmp_path / "bad.npy", clip.float().numpy())
    with pytest.raises(ValueError, match="uint8"):
        read_video(str(tmp_path / "bad.npy"))
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no images"):
        read_video(str(tmp_path / "empty"))


# ------------------------------------------------------------------------------------------ refusals of generate / generate_sample
SHAPE = (3, 8, 12, 16)


def call_generate(model=None, **kw):
    return generate(model or NS(visual_cond=True), "cpu", SHAPE, 4, None, None, None, None, None, 5.0, 5.0, None, noise=torch.zeros(SHAPE), **kw)


def test_generate_refuses_edit_controls_without_a_source():
    with pytest.raises(ValueError, match="init_latent"):
        call_generate(strength=0.5)
    with pytest.raises(ValueError, match="init_latent"):
        call_generate(keep_mask=torch.ones(3, 8, 12, 1))
    for s in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="strength"):
            call_generate(init_latent=torch.zeros(SHAPE), strength=s)
    with pytest.raises(ValueError, match="init_latent must be"):
        call_generate(init_latent=torch.zeros(3, 8, 12, 8))
    with pytest.raises(ValueError, match="keep_mask must be"):
        call_generate(init_latent=torch.zeros(SHAPE), keep_mask=torch.ones(3, 8, 12))


def test_generate_refuses_strength_below_one_under_magcache():
    for model in (NS(visual_cond=True, mag_ratios=[1.0] * 8), NS(visual_cond=True, mag_ratios=None, _magcache_calibrate=(4, False))):
        with pytest.raises(ValueError, match="step of a full run"):
            call_generate(model, init_latent=torch.zeros(SHAPE), strength=0.5)
        with pytest.raises(ValueError, match="step of a full run"):
            call_generate(model, init_latent=torch.zeros(SHAPE), strength=0.5, keep_mask=torch.ones(3, 8, 12, 1))


def test_generate_sample_refuses_edit_controls_without_a_video():
    args = ((1, 3, 8, 12, 16), "a cat", None, None, None, None)
    with pytest.raises(ValueError, match="video"):
        generate_sample(*args, strength=0.5)
    with pytest.raises(ValueError, match="video"):
        generate_sample(*args, mask=torch.ones(64, 96))
    with pytest.raises(ValueError, match="strength"):
        generate_sample(*args, video=torch.zeros(9, 64, 96, 3, dtype=torch.uint8), strength=0.0)


def test_cli_flags_reach_the_pipeline_keywords(tmp_path):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("k5_cli", os.path.join(root, "kandinsky-5_amd", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    clip = torch.randint(0, 256, (5, 16, 24, 3), dtype=torch.uint8)
    np.save(tmp_path / "clip.npy", clip.numpy())
    from PIL import Image
    keep = np.zeros((16, 24, 3), dtype=np.uint8)
    keep[:, :8] = 255
    Image.fromarray(keep).save(tmp_path / "keep.png")
    p = cli.build_parser()
    assert cli.load_edit_inputs(p.parse_args([])) == {}
    kw = cli.load_edit_inputs(p.parse_args(["--video", str(tmp_path / "clip.npy"), "--strength", "0.6", "--mask", str(tmp_path / "keep.png")]))
    assert torch.equal(kw["video"], clip) and kw["strength"] == 0.6
    # the mask file is resized and cropped like the frames: 16 x 24 -> the default 512 x 768 output, the left third white
    assert kw["mask"].shape == (512, 768) and (kw["mask"][:, :224] >= 0.99).all() and (kw["mask"][:, 288:] <= 0.01).all()
    small = cli.load_edit_inputs(p.parse_args(["--video", str(tmp_path / "clip.npy"), "--mask", str(tmp_path / "keep.png"), "--width", "512"]))
    assert small["mask"].shape == (512, 512) and "strength" not in small
    with pytest.raises(ValueError, match="--video"):
        cli.load_edit_inputs(p.parse_args(["--strength", "0.5"]))
