"""The BraTS22 3D U-Net of the reference (PyTorch/Segmentation/nnUNet/nnunet/brats22_model.py, UNet3D) as a layer table over a flat
state dict: no nn.Module.  get_unet_params restates nn_unet.py:139-159; the checkpoint reader takes the Lightning .ckpt the
reference writes (`state_dict` under the `model.` prefix) without pytorch_lightning: pickled foreign classes resolve to stand-ins.

Envelope of the kernels (csrc/nnunet.hip): every kernel 3x3x3, strides [1, 2, 2, ...] on all three axes, filters in multiples of 64.
MONAI's DynUNet (any run without --brats22_model), the 2-D model and anisotropic kernels / strides are turned away with one line.
"""
import io
import pickle

import torch

FILTERS = (64, 128, 256, 512, 768, 1024, 2048)
IN_CHANNELS, STEM_CHANNELS, N_CLASS = 5, 8, 3
EPS = 1e-5                                             # nn.InstanceNorm3d's default
# data_preprocessing/configs.py: the BraTS tasks (11: training data, 12: validation data) -- patch 128^3, spacing 1
TASK_CONFIG = {
    "11": {"patch_size": [128, 128, 128], "spacings": [1.0, 1.0, 1.0], "in_channels": 5, "n_class": 4},
    "12": {"patch_size": [128, 128, 128], "spacings": [1.0, 1.0, 1.0], "in_channels": 5, "n_class": 4},
}


class NNUnetConfigError(ValueError):
    """A configuration outside what is built; the message is one line."""


def get_unet_params(patch_size, spacings, depth=5, min_fmap=4):
    """(kernels, strides) per level, the rule of nn_unet.py:139-159.  Level 0 has stride 1.  Every further level halves the axes that
    are still fine-grained (spacing at most twice the finest) and at least 2 min_fmap voxels long, with kernel 3 on the fine-grained
    axes and 1 on the others; the spacing of a halved axis doubles.  Levels are added until no axis can be halved or `depth` of them
    exist; the last level (the bottleneck's) has kernel 3 everywhere."""
    axes = range(len(patch_size))
    extent, spacing = [float(e) for e in patch_size], [float(s) for s in spacings]
    kernels, strides = [], [[1 for _ in axes]]
    while True:
        fine = [spacing[a] / min(spacing) <= 2 for a in axes]
        step = [2 if fine[a] and extent[a] >= 2 * min_fmap else 1 for a in axes]
        if max(step) == 1:
            break
        kernels.append([3 if fine[a] else 1 for a in axes])
        strides.append(step)
        extent = [extent[a] / step[a] for a in axes]
        spacing = [spacing[a] * step[a] for a in axes]
        if len(kernels) == depth:
            break
    kernels.append([3 for _ in axes])
    return kernels, strides


def check_envelope(kernels, strides, dim=3):
    """-> number of levels, or NNUnetConfigError."""
    if dim != 3:
        raise NNUnetConfigError("nnU-Net: --dim 2 is not built (the BraTS22 UNet3D is volumetric)")
    kernels, strides = [list(k) for k in kernels], [list(s) for s in strides]
    if len(kernels) != len(strides) or not 2 <= len(strides) <= len(FILTERS):
        raise NNUnetConfigError("nnU-Net: %d kernel and %d stride levels; 2 to %d matching levels are built" % (len(kernels), len(strides), len(FILTERS)))
    if any(k != [3, 3, 3] for k in kernels):
        raise NNUnetConfigError("nnU-Net: kernels %s are outside the envelope (3x3x3 only; anisotropic MSD tasks are not built)" % kernels)
    if strides[0] != [1, 1, 1] or any(s != [2, 2, 2] for s in strides[1:]):
        raise NNUnetConfigError("nnU-Net: strides %s are outside the envelope ([1,1,1] then [2,2,2] per level)" % strides)
    return len(strides)


def conv_names(levels):
    """The convolutions in execution order: (weight key, norm key prefix or None, stride, C_in, C_out)."""
    f = FILTERS[:levels]
    out = [("input_block.conv1.weight", None, 1, IN_CHANNELS, f[0]), ("input_block.conv2.weight", "input_block.norm", 1, f[0], f[0])]
    blocks = [("downsamples.%d" % (i - 1), f[i - 1], f[i], 2) for i in range(1, levels - 1)] + [("bottleneck", f[-2], f[-1], 2)]
    blocks += [("upsamples.%d.conv_block" % j, f[levels - 1 - j] + f[levels - 2 - j], f[levels - 2 - j], 1) for j in range(levels - 1)]
    for name, cin, cout, stride in blocks:
        out.append((name + ".conv1.conv.weight", name + ".conv1.norm", stride, cin, cout))
        out.append((name + ".conv2.conv.weight", name + ".conv2.norm", 1, cout, cout))
    return out


def state_shapes(levels):
    """name -> shape of UNet3D's state dict, in its order."""
    f, ordered = FILTERS[:levels], {}
    for key, norm, _, cin, cout in conv_names(levels):
        # registration order: a ConvLayer's conv, then its norm over the INPUT channels; InputBlock's conv1, conv2, then its norm
        # over its OUTPUT channels (it sits between the two convolutions)
        ordered[key] = (cout, cin, 3, 3, 3)
        if norm is not None:
            ordered[norm + ".weight"] = ordered[norm + ".bias"] = (f[0],) if norm == "input_block.norm" else (cin,)
    ordered["output_block.conv.weight"] = (N_CLASS, f[0], 1, 1, 1)
    ordered["output_block.conv.bias"] = (N_CLASS,)
    for i in range(2 if levels >= 3 else 0):           # (UNet3D itself cannot be built with fewer than three levels: filters[2])
        ordered["deep_supervision_heads.%d.conv.weight" % i] = (N_CLASS, f[i + 1], 1, 1, 1)
        ordered["deep_supervision_heads.%d.conv.bias" % i] = (N_CLASS,)
    return ordered


def levels_of(state):
    """Number of levels of a UNet3D state dict; DynUNet key sets and anything else are turned away."""
    keys = set(state)
    if any(k.startswith(("input_block.conv1.conv", "skip_layers", "downsamples.0.conv1.conv.conv")) or ".transp_conv" in k for k in keys):
        raise NNUnetConfigError("nnU-Net: this is a MONAI DynUNet state dict; only the BraTS22 UNet3D (--brats22_model) is built")
    if "input_block.conv1.weight" not in keys or "bottleneck.conv1.conv.weight" not in keys:
        raise NNUnetConfigError("nnU-Net: not a BraTS22 UNet3D state dict (input_block.conv1.weight / bottleneck.conv1.conv.weight missing)")
    levels = 2 + len({k.split(".")[1] for k in keys if k.startswith("downsamples.")})
    want = state_shapes(levels)
    for name, shape in want.items():
        if name.startswith("deep_supervision_heads"):
            continue                                   # unused under eval()
        if name not in state:
            raise NNUnetConfigError("nnU-Net: state dict lacks %s" % name)
        if tuple(state[name].shape) != shape:
            raise NNUnetConfigError("nnU-Net: %s has shape %s, outside the envelope (expected %s)" % (name, tuple(state[name].shape), shape))
    return levels


def seeded_state(levels, seed=0):
    """UNet3D-shaped fp32 weights from a seeded generator, every value representable in fp16 (tests and benchmarks; the reference's
    kaiming_normal_ scale for the convolutions, non-trivial affine parameters so that a swapped gamma / beta shows)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in state_shapes(levels).items():
        if len(shape) == 5:
            fan_in = shape[1] * shape[2] * shape[3] * shape[4]
            t = torch.randn(shape, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5
        elif name.endswith("norm.weight"):
            t = 1.0 + 0.25 * torch.randn(shape, generator=g, dtype=torch.float64)
        else:
            t = 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
        out[name] = t.to(torch.float16).to(torch.float32)
    return out


def pack_conv_weight(w, dtype, device):
    """[Ko, C, 3, 3, 3] fp32 -> [Ko, 3, 3, 3, C'] 16-bit, the stem's 5 channels zero-padded to 8."""
    ko, c = w.shape[:2]
    w = w.to(device=device, dtype=torch.float32).permute(0, 2, 3, 4, 1)
    if c == IN_CHANNELS:
        w = torch.nn.functional.pad(w, (0, STEM_CHANNELS - c))
    return w.to(dtype).contiguous()


# ---------------------------------------------------------------------------------------------- checkpoint
class _Stub:
    """Stand-in for a pickled class of a package that is not installed (pytorch_lightning's AttributeDict, argparse extras...)."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        self.__dict__.update(state if isinstance(state, dict) else {"state": state})


class _StubDict(dict):
    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)


# Classes of these packages are loaded as they are; of `builtins` only the plain containers and scalars a checkpoint holds.  Every
# other name (a foreign package's class, or a builtin such as eval) becomes an inert stand-in.  This keeps a checkpoint readable
# without its packages; it is not a sandbox -- read checkpoints you trust, as with torch.load itself.
_REAL_PACKAGES = ("torch", "collections", "numpy", "argparse", "_codecs")
_REAL_BUILTINS = ("set", "frozenset", "dict", "list", "tuple", "int", "float", "bool", "str", "bytes", "bytearray", "complex", "slice", "range",
                  "object")


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.split(".")[0] in _REAL_PACKAGES or (module == "builtins" and name in _REAL_BUILTINS):
            return super().find_class(module, name)
        return _StubDict if "Dict" in name else type(name, (_Stub,), {"__module__": module})


class _PickleModule:
    __name__ = "pickle"
    Unpickler = _Unpickler
    load = staticmethod(lambda f, **kw: _Unpickler(f, **kw).load())
    loads = staticmethod(lambda b, **kw: _Unpickler(io.BytesIO(b), **kw).load())
    dumps, dump = pickle.dumps, pickle.dump


def load_checkpoint(path):
    """-> (state dict of UNet3D as fp32 CPU tensors, hyper-parameter dict or {}) from the reference's Lightning .ckpt (or from a bare
    state dict file)."""
    ckpt = torch.load(path, map_location="cpu", pickle_module=_PickleModule, weights_only=False)
    sd = ckpt.get("state_dict", ckpt) if isinstance(ckpt, dict) else None
    if not isinstance(sd, dict) or not sd:
        raise NNUnetConfigError("nnU-Net: %s holds no state_dict" % path)
    state = {(k[len("model."):] if k.startswith("model.") else k): v.detach().to(torch.float32) for k, v in sd.items() if torch.is_tensor(v)}
    hp = ckpt.get("hyper_parameters", {}) if isinstance(ckpt, dict) else {}
    args = hp.get("args") if isinstance(hp, dict) else None
    hp = dict(vars(args)) if args is not None and hasattr(args, "__dict__") else (dict(hp) if isinstance(hp, dict) else {})
    levels_of(state)
    return state, hp
