"""Saving results (reference t2v_pipeline.py:166-189 uses torchvision.io.write_video / ToPILImage; neither
torchvision nor PyAV exists in the ROCm image).  write_video tries torchvision, then PyAV, and otherwise writes the
frames losslessly as an animated PNG next to the requested path (same base name, .png) so nothing is silently lost."""
import os

import torch


def to_pil_images(images):
    """(B,3,H,W) uint8 -> list of PIL images."""
    from PIL import Image
    return [Image.fromarray(img.permute(1, 2, 0).contiguous().numpy()) for img in images]


def write_video(path, frames, fps=24, crf="5"):
    """frames (T,H,W,3) uint8 (CPU).  Returns the path actually written."""
    frames = frames.to(torch.uint8).contiguous()
    try:
        import torchvision
        torchvision.io.write_video(path, frames.numpy(), fps=fps, options={"crf": str(crf)})
        return path
    except Exception:
        pass
    try:
        import av
        with av.open(path, mode="w") as container:
            stream = container.add_stream("libx264", rate=fps)
            stream.height, stream.width = frames.shape[1], frames.shape[2]
            stream.options = {"crf": str(crf)}
            for f in frames.numpy():
                for packet in stream.encode(av.VideoFrame.from_ndarray(f, format="rgb24")):
                    container.mux(packet)
            for packet in stream.encode():
                container.mux(packet)
        return path
    except Exception:
        pass
    from PIL import Image
    out = os.path.splitext(path)[0] + ".png"
    imgs = [Image.fromarray(f) for f in frames.numpy()]
    imgs[0].save(out, save_all=True, append_images=imgs[1:], duration=int(round(1000 / fps)), loop=0)
    return out


_IMAGE_EXT = (".png", ".apng", ".gif", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff")


def read_video(path):
    """A clip as uint8 (F,H,W,3) on the CPU.  `path`: a `.npy` / `.pt` file holding (F,H,W,3) uint8; a directory of images, read in
    name order; a container, through torchvision, then PyAV (as `write_video` tries them); an animated PNG / GIF (or any still image:
    one frame) through PIL — what `write_video`'s fallback writes, so a clip written here reads back."""
    import numpy as np
    if os.path.isdir(path):
        from PIL import Image
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(_IMAGE_EXT))
        if not names:
            raise ValueError(f"no images in {path}")
        frames = [np.asarray(Image.open(os.path.join(path, n)).convert("RGB"), dtype=np.uint8) for n in names]
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError(f"the images in {path} differ in size")
        return torch.from_numpy(np.stack(frames))
    ext = os.path.splitext(path)[1].lower()
    if ext in (".npy", ".pt"):
        data = torch.from_numpy(np.load(path)) if ext == ".npy" else torch.load(path, map_location="cpu")
        if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.dim() != 4 or data.shape[-1] != 3:
            raise ValueError(f"{path} must hold a uint8 (F,H,W,3) array, got {getattr(data, 'dtype', type(data))} "
                             f"{tuple(getattr(data, 'shape', ()))}")
        return data.contiguous()
    if ext not in _IMAGE_EXT:
        try:
            import torchvision
            frames = torchvision.io.read_video(path, pts_unit="sec", output_format="THWC")[0]
            if frames.numel():
                return frames.to(torch.uint8).contiguous()
        except Exception:
            pass
        try:
            import av
            with av.open(path) as container:
                frames = [f.to_ndarray(format="rgb24") for f in container.decode(video=0)]
            if frames:
                return torch.from_numpy(np.stack(frames))
        except Exception:
            pass
    from PIL import Image, ImageSequence
    with Image.open(path) as im:
        frames = [np.asarray(f.convert("RGB"), dtype=np.uint8) for f in ImageSequence.Iterator(im)]
    return torch.from_numpy(np.stack(frames))
