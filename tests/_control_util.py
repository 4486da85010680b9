"""Shared helpers of the ControlNet tests (test_control_cpu.py, test_controlnet_gpu.py, test_control_sampling_gpu.py).

ControlOracle restates cldm.py of the ControlNet paper's repository (ControlNet.forward, ControlledUnetModel.forward) WITHOUT
touching oracle/: it is built from oracle.ldm's UNetOracle._layer, conv2d, silu, dense and timestep_embedding.

    g     = input_hint_block(hint)                  eight 3x3 convs (pad 1), SiLU after every one but the last
    h     = input_blocks[0](x) + g;  r_i = zero_convs[i](h) after input block i;  r_mid = middle_block_out(h)
    UNet:   hs[i] as usual;  h = middle(h) + r_mid;  output block k reads cat([h, hs.pop() + control.pop()])

rows / scale are the tables of the product's add: residual i reaches UNet batch row r as scale[i][r] * r_i[rows[r]], or not at
all when rows[r] is -1.  With a gain of 1 on the hint path the hint moves eps by ~4e-3 -- under the parity tolerance -- so the
synthetic weights multiply the last hint conv by HINT_GAIN (test_control_cpu.py asserts what that buys).
"""
import math

import numpy as np
import torch

from oracle import ldm as O

HINT_LAYERS = ((16, 1), (16, 1), (32, 2), (32, 1), (96, 2), (96, 1), (256, 2))      # (cout, stride) but the last conv
HINT_GAIN = 32.0


def hint_convs(cfg, hint_channels=3):
    """(cin, cout, stride) of the eight hint convs."""
    chans = [c for c, _ in HINT_LAYERS] + [cfg["model_channels"]]
    strides = [s for _, s in HINT_LAYERS] + [1]
    return list(zip([hint_channels] + chans[:-1], chans, strides))


def block_channels(cfg):
    out = []
    for blk in O.unet_structure(cfg)[0]:
        last = blk[-1]
        out.append(last[1] if last[0] in ("st", "down") else last[2])
    return out


def control_param_shapes(cfg, hint_channels=3):
    """name -> shape of a ControlNet for the UNet config `cfg` (oracle form: num_heads=-1 where head channels are given)."""
    s = {k: v for k, v in O.unet_param_shapes(cfg).items() if not k.startswith(("output_blocks.", "out.", "id_predictor."))}
    for k, (cin, cout, _) in enumerate(hint_convs(cfg, hint_channels)):
        s[f"input_hint_block.{2 * k}.conv.weight"] = (cout, cin, 3, 3)
        s[f"input_hint_block.{2 * k}.conv.bias"] = (cout,)
    chans = block_channels(cfg)
    for pre, ch in [(f"zero_convs.{i}.0.", ch) for i, ch in enumerate(chans)] + [("middle_block_out.0.", chans[-1])]:
        s[pre + "conv.weight"] = (ch, ch, 1, 1)
        s[pre + "conv.bias"] = (ch,)
    return s


def init_control_params(cfg, seed=1, hint_channels=3, zero=False, gain=HINT_GAIN):
    """Seeded synthetic ControlNet weights in the style of O.init_params: fan-in-scaled normals.  zero=True: the zero convs
    as the paper initialises them (weights and biases 0).  The last hint conv's weight is multiplied by `gain`."""
    rng = np.random.RandomState(seed)
    params = {}
    for name, shape in control_param_shapes(cfg, hint_channels).items():
        if name.endswith(".gamma"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif name.endswith(".beta"):
            v = 0.1 * rng.standard_normal(shape)
        elif name.endswith(".bias"):
            v = 0.05 * rng.standard_normal(shape)
        else:
            v = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[1:])))
        if name == "input_hint_block.14.conv.weight":
            v = v * gain
        if zero and name.startswith(("zero_convs.", "middle_block_out.")):
            v = np.zeros(shape)
        params[name] = v.astype(np.float32)
    return params


def full_rows(nb):
    return list(range(nb))


def scale_table(scale, n_res, b, nb):
    """[n_res, nb] float64 from a float, a per-sample list [b], a per-residual list [n_res] or a table [n_res, b]."""
    s = np.asarray(scale, dtype=np.float64)
    if s.ndim == 0:
        tab = np.full((n_res, b), float(s))
    elif s.ndim == 2:
        tab = s
    elif len(s) == n_res:
        tab = np.repeat(s[:, None], b, 1)
    else:
        assert len(s) == b
        tab = np.repeat(s[None, :], n_res, 0)
    return np.tile(tab, (1, nb // b))


class ControlOracle:
    """fp32 CPU restatement of a ControlNet and of the UNet forward that consumes its residuals."""

    def __init__(self, cfg, unet_params, control_params, hint_channels=3):
        self.cfg = dict(cfg)
        self.unet = O.UNetOracle(cfg, unet_params)
        self.cn = O.UNetOracle(cfg, control_params)          # input_blocks / middle_block / time_embed of the ControlNet
        self.hint_channels = hint_channels
        self.n_res = len(self.unet.input_blocks) + 1

    @staticmethod
    def _emb(net, timesteps):
        p = net.p
        t_emb = O.timestep_embedding(torch.as_tensor(timesteps), net.cfg["model_channels"])
        emb = O.dense(t_emb, p["time_embed.0.weight"], p["time_embed.0.bias"])
        return O.dense(O.silu(emb), p["time_embed.2.weight"], p["time_embed.2.bias"])

    @torch.no_grad()
    def hint_features(self, hint):
        """input_hint_block: [B, hc, 8h, 8w] -> [B, model_channels, h, w]."""
        p = self.cn.p
        g = O.r16(torch.as_tensor(hint, dtype=torch.float32))
        convs = hint_convs(self.cfg, self.hint_channels)
        for k, (_, _, stride) in enumerate(convs):
            g = O.conv2d(g, p[f"input_hint_block.{2 * k}.conv.weight"], p[f"input_hint_block.{2 * k}.conv.bias"], stride=stride)
            if k != len(convs) - 1:
                g = O.silu(g)
        return g

    @torch.no_grad()
    def residuals(self, x, timesteps, context, hint):
        """ControlNet.forward: the n_res residuals, NCHW, input blocks first, the middle block's last."""
        net, p = self.cn, self.cn.p
        x = O.r16(torch.as_tensor(x, dtype=torch.float32))
        context = O.r16(torch.as_tensor(context, dtype=torch.float32))
        emb = self._emb(net, timesteps)
        g = self.hint_features(hint)
        out, h = [], x
        for i, block in enumerate(net.input_blocks):
            for j, layer in enumerate(block):
                h = net._layer(f"input_blocks.{i}.{j}.", layer, h, emb, context)
            if i == 0:
                h = O.r16(h + g)
            out.append(O.conv2d(h, p[f"zero_convs.{i}.0.conv.weight"], p[f"zero_convs.{i}.0.conv.bias"], padding=0))
        for j, layer in enumerate(net.middle):
            h = net._layer(f"middle_block.{j}.", layer, h, emb, context)
        out.append(O.conv2d(h, p["middle_block_out.0.conv.weight"], p["middle_block_out.0.conv.bias"], padding=0))
        return out

    @torch.no_grad()
    def unet_forward(self, x, timesteps, context, control=None, rows=None, scale=None):
        """ControlledUnetModel.forward.  control: the residual list (or None: the plain UNet); rows[r]: the residual row added
        to batch row r (-1: none; default: row r); scale: [n_res, NB] (default: 1)."""
        net, p = self.unet, self.unet.p
        x = O.r16(torch.as_tensor(x, dtype=torch.float32))
        context = O.r16(torch.as_tensor(context, dtype=torch.float32))
        NB = x.shape[0]
        emb = self._emb(net, timesteps)
        if control is not None:
            rows = full_rows(NB) if rows is None else list(rows)
            scale = np.ones((len(control), NB)) if scale is None else np.asarray(scale, dtype=np.float64)

        def add(h, i):
            if control is None:
                return h
            out = h.clone()
            for r, q in enumerate(rows):
                if q >= 0:
                    out[r] = O.r16(h[r] + float(np.float32(scale[i][r])) * control[i][q])
            return out
        hs, h = [], x
        for i, block in enumerate(net.input_blocks):
            for j, layer in enumerate(block):
                h = net._layer(f"input_blocks.{i}.{j}.", layer, h, emb, context)
            hs.append(h)
        for j, layer in enumerate(net.middle):
            h = net._layer(f"middle_block.{j}.", layer, h, emb, context)
        h = add(h, len(hs))
        for i, block in enumerate(net.output_blocks):
            k = len(hs) - 1
            h = torch.cat([h, add(hs.pop(), k)], dim=1)
            for j, layer in enumerate(block):
                h = net._layer(f"output_blocks.{i}.{j}.", layer, h, emb, context)
        h = O.silu(O.group_norm(h, p["out.0.gamma"], p["out.0.beta"], 1e-5))
        return O.conv2d(h, p["out.2.conv.weight"], p["out.2.conv.bias"])

    def controlled(self, x, timesteps, context, hint, scale=1.0, uncond=True, guided=False, permute=None):
        """One controlled model call.  guided: the batch is [uncond ; cond] of b = NB / 2 samples; uncond=False then runs the
        ControlNet on the conditional half only and leaves the unconditional rows alone.  hint: [b | NB | 1, ...].  permute: a
        permutation of the residual list (the discrimination checks swap two same-shaped residuals)."""
        x = torch.as_tensor(x, dtype=torch.float32)
        context = torch.as_tensor(context, dtype=torch.float32)
        timesteps = torch.as_tensor(timesteps)
        hint = torch.as_tensor(hint, dtype=torch.float32)
        NB = x.shape[0]
        b = NB // 2 if guided else NB
        half = guided and not uncond
        n_cn = b if half else NB
        if hint.shape[0] == 1:
            hint = hint.expand(n_cn, -1, -1, -1)
        elif hint.shape[0] != n_cn:
            hint = torch.cat([hint] * (n_cn // hint.shape[0]), 0)
        sl = slice(b, None) if half else slice(None)
        res = self.residuals(x[sl], timesteps[sl], context[sl], hint)
        if permute is not None:
            res = [res[k] for k in permute]
        rows = ([-1] * b + list(range(b))) if half else full_rows(NB)
        return self.unet_forward(x, timesteps, context, res, rows, scale_table(scale, self.n_res, b, NB))


class ControlledUNet:
    """A ControlOracle with a fixed hint / scale / uncond behind UNetOracle's call signature: the `unet` of any ModelOracle
    (plain, v-prediction, rescaled).  b: samples per batch -- a call on 2 b rows is the guidance batch [uncond ; cond]."""

    def __init__(self, oracle, hint, b, scale=1.0, uncond=True):
        self.oracle, self.hint, self.b, self.scale, self.uncond = oracle, hint, int(b), scale, bool(uncond)
        self.cfg = oracle.cfg

    def __call__(self, x, timesteps, context=None, y=None):
        assert y is None and context is not None
        guided = int(torch.as_tensor(x).shape[0]) == 2 * self.b
        return self.oracle.controlled(x, timesteps, context, self.hint, self.scale, self.uncond, guided)

    forward = __call__


class ControlModelOracle(O.ModelOracle):
    """O.ModelOracle whose apply_model goes through ControlOracle.controlled (a 'crossattn' model)."""

    def __init__(self, oracle, hint, b, scale=1.0, uncond=True, **kw):
        super().__init__(ControlledUNet(oracle, hint, b, scale, uncond), conditioning_key="crossattn", **kw)

    def apply_model(self, x, t, cond=None):
        self.calls += 1
        return self.unet(x, t, cond)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / (np.sqrt((b ** 2).sum()) + 1e-30))


def blocky_hint(rng, B, hint_channels, Hh, Wh, block=4):
    """A hint as ControlNet hints are -- edge maps, scribbles, segmentation: piecewise constant in {0, 1} -- here random
    `block`-pixel squares.  Per-pixel noise would be averaged away by the three stride-2 convs of the hint block; a
    piecewise-constant image reaches the latent grid."""
    coarse = (rng.rand(B, hint_channels, -(-Hh // block), -(-Wh // block)) > 0.5).astype(np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, 2), block, 3)[:, :, :Hh, :Wh])


def inputs(cfg, B=2, H=8, W=8, T=6, seed=301, hint_channels=3):
    """x, t, context and a hint in [0, 1] for a B x H x W latent batch."""
    rng = np.random.RandomState(seed)
    x = rng.randn(B, cfg["in_channels"], H, W).astype(np.float32)
    t = np.asarray([500, 37] * B, dtype=np.int64)[:B]
    c = rng.randn(B, T, cfg["context_dim"]).astype(np.float32)
    return x, t, c, blocky_hint(rng, B, hint_channels, 8 * H, 8 * W)


def nchw(t, C, H, W):
    """NHWC fp16 [B, H * W, C'] device buffer -> NCHW fp32 numpy [B, C, H, W]."""
    t = t.detach().float().cpu()
    B = t.shape[0]
    return t.reshape(B, H, W, -1)[..., :C].permute(0, 3, 1, 2).contiguous().numpy()
