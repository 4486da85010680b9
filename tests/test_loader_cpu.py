"""The shared weight loader (minddiffusion_amd/loader.py) on the host: what every class raises for a missing key, an unexpected
key and a wrong shape, and the consistency of parameter_shapes() with the names load_state_dict reads.

EXPECTED was recorded by running outcome() below on the commit BEFORE the classes moved onto the shared loader, not from the
new code.  Three entries differ from that run on purpose: Decoder, Encoder and AutoencoderKL with strict=False and a needed key
missing ended in a bare KeyError from the dict lookup a few lines after the skipped check; they now raise the halves' own
MdxError, which names the key as well."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import weights_fingerprint as WF  # noqa: E402

TABLE = WF.case_table()
FAULTS = ("missing", "unexpected", "shape")
# one case per class (both GLIDE models, both VAE halves as AutoencoderKL calls them, both PReLU spellings)
CLASS_CASES = ("tiny_unet", "tiny_unet lora + adapter", "tiny_glide base", "tiny_glide upsampler",
               "tiny_vae decoder post_quant prefix", "tiny_vae encoder quant prefix", "tiny_vae", "tiny_text_encoder",
               "frozen_embedder", "srgan x2 .a float32", "srgan x4 .w float32")


def outcome(case, fault, strict):
    """Load with one fault -> (exception class name, whether the message names the key), or (None, None) when it loads."""
    params = dict(case.params)
    key = [k for k in case.shapes if k in params][-1]
    if fault == "missing":
        del params[key]
    elif fault == "unexpected":
        key = "bogus.key"
        params[key] = np.zeros(1, np.float32)
    else:
        params[key] = np.zeros(tuple(case.shapes[key]) + (2,), np.float32)
    try:
        case.load(params, strict=strict)
    except Exception as e:
        return type(e).__name__, key in str(e)
    return None, None


_KEY, _VAL, _MDX = ("KeyError", True), ("ValueError", True), ("MdxError", True)
_OK = (None, None)
# class of cases -> {(fault, strict): outcome}
_PLAIN = {("missing", True): _KEY, ("missing", False): _KEY, ("unexpected", True): _KEY, ("unexpected", False): _OK,
          ("shape", True): _VAL, ("shape", False): _VAL}
_HALF = {("missing", True): _MDX, ("missing", False): _MDX,       # strict=False: a bare KeyError before (see the docstring)
         ("unexpected", True): _OK, ("unexpected", False): _OK, ("shape", True): _MDX, ("shape", False): _MDX}
_SRGAN = {("missing", True): _MDX, ("missing", False): _MDX, ("unexpected", True): _MDX, ("unexpected", False): _OK,
          ("shape", True): _MDX, ("shape", False): _MDX}
EXPECTED = {"tiny_unet": _PLAIN, "tiny_unet lora + adapter": _PLAIN, "tiny_glide base": _PLAIN, "tiny_glide upsampler": _PLAIN,
            "tiny_text_encoder": _PLAIN, "frozen_embedder": _PLAIN,
            "tiny_vae decoder post_quant prefix": _HALF, "tiny_vae encoder quant prefix": _HALF,
            # strict: AutoencoderKL's own check of the whole dict; otherwise the halves'
            "tiny_vae": {("missing", True): _KEY, ("missing", False): _MDX, ("unexpected", True): _KEY, ("unexpected", False): _OK,
                         ("shape", True): _VAL, ("shape", False): _MDX},
            "srgan x2 .a float32": _SRGAN, "srgan x4 .w float32": _SRGAN}


@pytest.mark.parametrize("name", CLASS_CASES)
def test_every_class_raises_what_it_raised_before(name):
    case = WF.build_case(name, TABLE)
    for fault in FAULTS:
        for strict in (True, False):
            assert outcome(case, fault, strict) == EXPECTED[name][fault, strict], (fault, strict)


def test_srgan_names_both_prelu_spellings():
    from minddiffusion_amd._lib import MdxError
    case = WF.build_case("srgan x4 .w float32", TABLE)
    params = {k: v for k, v in case.params.items() if k != "trunk.2.prelu.w"}
    with pytest.raises(MdxError, match=r"trunk\.2\.prelu\.a \(or trunk\.2\.prelu\.w\)"):
        case.load(params)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_parameter_shapes_cover_what_the_load_reads(name):
    """load_state_dict ends in WeightLoader.finish(): every name of parameter_shapes() the class runs on was read and every
    name read is in parameter_shapes() -- for every configuration of the fingerprint list."""
    case = WF.build_case(name, TABLE)
    case.load()
    assert all(w for _, w in case.weights())


def test_a_name_dropped_from_parameter_shapes_is_caught():
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.loader import LoaderMismatch
    from minddiffusion_amd.weights import synthetic_unet_params_numpy

    class Forgetful(UNetModel):
        def parameter_shapes(self):
            s = super().parameter_shapes()
            del s["middle_block.0.in_layers_norm.beta"]
            return s
    params = synthetic_unet_params_numpy(UNetModel(device="cpu", **TINY_UNET).parameter_shapes())
    with pytest.raises(LoaderMismatch, match=r"middle_block\.0\.in_layers_norm\.beta"):
        Forgetful(device="cpu", **TINY_UNET).load_state_dict(params, strict=False)


def test_a_name_the_load_never_reads_is_caught():
    from minddiffusion_amd.ldm.modules.encoders.text_encoder import TextEncoder
    from minddiffusion_amd.loader import LoaderMismatch

    class Padded(TextEncoder):
        def parameter_shapes(self, prefix=""):
            return dict(super().parameter_shapes(prefix), **{prefix + "text_projection": (self.width, self.width)})
    enc = Padded(context_length=8, vocab_size=10, output_dim=64, width=64, layers=1, heads=1, device="cpu")
    params = {k: np.zeros(s, np.float32) for k, s in enc.parameter_shapes().items()}
    with pytest.raises(LoaderMismatch, match="text_projection"):
        enc.load_state_dict(params)


def test_loader_conversion_routes():
    """Both routes are kept as the classes had them: the direct one is ``t.to(device, dtype)``, the SRGAN one rounds a float64
    input to float32 on the host first, then to float16.  For float32 and float16 inputs the two give the same bits."""
    import torch
    from minddiffusion_amd.loader import WeightLoader
    x = np.array([1.0 + 2.0 ** -11 + 2.0 ** -30], np.float64)        # above the float16 tie, on it after rounding to float32
    via = WeightLoader({"x": x}, "cpu", "t", via_f32=True).raw("x", torch.float16)
    assert float(via) == 1.0                                         # the tie goes to even
    direct = WeightLoader({"x": x}, "cpu", "t").raw("x", torch.float16)
    assert torch.equal(direct, torch.from_numpy(x).to(torch.float16))
    for dtype in (np.float32, np.float16):
        y = np.random.RandomState(0).standard_normal(64).astype(dtype)
        a = WeightLoader({"y": y}, "cpu", "t").raw("y", torch.float16)
        b = WeightLoader({"y": y}, "cpu", "t", via_f32=True).raw("y", torch.float16)
        assert torch.equal(a, b)
