"""SRGAN front end of Taichu-GLIDE's CLI (vision/Taichu-GLIDE/model/glide_text2im/model/srgan_util.py:25-61): the checkpoint
loader around the Generator, sr_handle (tensor in, tensor out), sr_image (PNG in, PNG out) and get_img (the uint8 strip the CLI
saves)."""
import warnings

import numpy as np
import torch

from ..._lib import MdxError
from .srgan import Generator


def get_img(batch):
    """srgan_util.py:25-33: [B, 3, H, W] in [-1, 1] -> uint8 [H, B * W, 3] = clip(rint((x + 1) * 127.5), 0, 255) (rint rounds
    halves to even, as ops.Rint does).  The arithmetic runs in the input's precision (float64 stays float64, anything else fp32), as
    the reference's Add / Mul keep the tensor's dtype."""
    x = batch.detach().cpu().numpy() if isinstance(batch, torch.Tensor) else np.asarray(batch)
    ft = np.float64 if x.dtype == np.float64 else np.float32
    x = np.clip(np.rint((x.astype(ft) + ft(1)) * ft(127.5)), 0, 255)
    x = x.transpose(2, 0, 3, 1).astype(np.uint8)
    return x.reshape(x.shape[0], -1, 3)


class SRGAN:
    def __init__(self, upscale_factor, ckpt_path=None, device=None, use_graph=True, params=None):
        """ckpt_path: a MindSpore .ckpt of the Generator (reference names).  `params` (a name -> array dict) may be given
        instead.  Unexpected keys warn; a missing key raises MdxError naming it."""
        self.net = Generator(upscale_factor, device=device, use_graph=use_graph)
        if params is None:
            if ckpt_path is None:
                raise MdxError("SRGAN: ckpt_path (or params) is required")
            from ...ms_checkpoint import load_checkpoint
            params = load_checkpoint(ckpt_path)
        params = self.net.normalize_keys(params)
        own = self.net.parameter_shapes()
        self.unexpected_keys = sorted(k for k in params if k not in own)
        if self.unexpected_keys:
            warnings.warn(f"SRGAN: {len(self.unexpected_keys)} checkpoint keys are not parameters of the Generator and were "
                          f"ignored: {self.unexpected_keys[:8]}{' ...' if len(self.unexpected_keys) > 8 else ''}")
        self.net.load_state_dict({k: v for k, v in params.items() if k in own}, strict=True)

    def sr_handle(self, lr):
        """srgan_util.py:45-47: fp32 NCHW [B, 3, H, W] on the GPU -> fp32 NCHW [B, 3, f H, f W] (tanh range).  The result is a
        fresh tensor (the plan's output buffer is copied)."""
        return self.net(lr).clone()

    def sr_image(self, lr_image, hr_image):
        """srgan_util.py:50-61: PNG / JPEG file -> x f upscaled image file."""
        from PIL import Image
        lr = np.array(Image.open(lr_image).convert("RGB"))
        lr = (lr / 127.5) - 1.0
        lr = lr.transpose(2, 0, 1).astype(np.float32)[None]
        out = self.sr_handle(torch.from_numpy(lr).to(self.net.device)).cpu().numpy()[0]
        out = np.clip(out, -1.0, 1.0)
        out = (out + 1.0) / 2.0
        out = out.transpose(1, 2, 0)
        Image.fromarray((out * 255.0).astype(np.uint8)).save(hr_image, quality=100)
        return hr_image

    @staticmethod
    def get_img(batch):
        return get_img(batch)
