"""Jasper's parameters under the reference's names (SpeechRecognition/Jasper/jasper/model.py:88-257: JasperBlock, JasperEncoder,
JasperDecoderForCTC, Jasper) and its configuration as the reference's YAML holds it (configs/jasper10x5dr_speedp-online_speca.yaml:
`labels`, `input_val.filterbank_features`, `jasper.encoder`, `jasper.decoder`).

A container, not a module: it holds the tensors of `Jasper(encoder_kw, decoder_kw).state_dict()` --
  encoder.layers.N.conv.M.*   sub-block r of block N is conv.{4r} (MaskedConv1d weight [Ko, C, K]) and conv.{4r + 1} (BatchNorm1d:
                              weight, bias, running_mean, running_var, num_batches_tracked); 4r + 2 / 4r + 3 are the activation and
                              the dropout (no tensors, absent behind the last sub-block);
  encoder.layers.N.res.J.0.weight [Ko, C_J, 1], encoder.layers.N.res.J.1.*   residual pane J (1x1 conv, BatchNorm1d);
  decoder.layers.0.weight [n_classes, C, 1], decoder.layers.0.bias
-- and has no forward: that lives in jasper/infer.py.

Dense residuals (JasperEncoder.__init__, model.py:185-200; JasperBlock.forward, :137-166).  The encoder carries a LIST of
activations.  A block with `residual_dense` reads every entry of the list through a 1x1 convolution + BatchNorm of its own (its
panes) and appends its output; the i-th dense block of a run therefore has i panes, whose widths are the inputs of the dense
blocks so far.  A block with `residual: true` and no `residual_dense` has one pane, its own input; it and a block with `residual:
false` hand on their output alone, so the list starts again behind them.
"""
import collections
import re

from ..quartznet.model import QuartzNetModel, _bn_shapes, _one, apply_overrides      # noqa: F401 (apply_overrides: for the CLI)
from ..utils.state import strip_module_prefix

BN_EPS = 1e-3                  # model.py:131
BLOCK_KEYS = ("filters", "repeat", "kernel_size", "stride", "dilation", "padding", "dropout", "residual", "residual_dense")


def residual_panes(blocks, in_feats):
    """blocks: dicts with `filters`, `residual`, `residual_dense` -> per block the list of its panes' input widths."""
    panes, run, c = [], [], int(in_feats)
    for blk in blocks:
        if not blk.get("residual", True):
            panes.append([])
            run = []
        elif blk.get("residual_dense", False):
            run = run + [c]
            panes.append(list(run))
        else:
            panes.append([c])
            run = []
        c = int(blk["filters"])
    return panes


def check_config(cfg):
    """What inference builds of a Jasper YAML -> (labels, features dict, list of block dicts with plain ints and `panes`).
    Everything else is rejected with a one-line message."""
    if "jasper" not in cfg or "encoder" not in cfg["jasper"]:
        raise ValueError("not a Jasper config: no jasper.encoder section")
    enc = cfg["jasper"]["encoder"]
    if enc.get("activation") != "relu":
        raise ValueError("activation %r: only relu is built" % (enc.get("activation"),))
    if not enc.get("use_conv_masks", False):
        raise ValueError("use_conv_masks false: only masked convolutions (variable-length batches) are built")
    if int(enc.get("frame_splicing", 1)) != 1:
        raise ValueError("frame_splicing %r: only 1 is built" % (enc.get("frame_splicing"),))
    feats = dict((cfg.get("input_val") or {}).get("filterbank_features") or {})
    if feats.get("normalize", "per_feature") != "per_feature":
        raise ValueError("normalize %r: only per_feature is built" % (feats.get("normalize"),))
    if int(feats.get("frame_splicing", 1)) != 1:
        raise ValueError("frame_splicing %r: only 1 is built" % (feats.get("frame_splicing"),))
    labels = list(cfg.get("labels") or [])
    if not labels:
        raise ValueError("the config holds no labels")
    raw = enc.get("blocks") or []
    if not raw:
        raise ValueError("the encoder has no blocks")
    for i, blk in enumerate(raw):
        for k in blk:
            if k not in BLOCK_KEYS:
                raise ValueError("block %d: unknown key %r" % (i, k))
        if blk.get("residual_dense", False) and not blk.get("residual", True):
            raise ValueError("block %d: residual_dense without residual" % i)
    panes = residual_panes(raw, enc["in_feats"])
    blocks = []
    c = int(enc["in_feats"])
    for i, blk in enumerate(raw):
        if blk.get("padding", "same") not in ("same", ["same"]):
            raise ValueError("block %d: only 'same' padding is built" % i)
        b = dict(infilters=c, filters=int(blk["filters"]), repeat=int(blk.get("repeat", 3)),
                 kernel_size=_one(blk.get("kernel_size", 11), "kernel_size"), stride=_one(blk.get("stride", 1), "stride"),
                 dilation=_one(blk.get("dilation", 1), "dilation"), residual=bool(blk.get("residual", True)),
                 dense=bool(blk.get("residual", True) and blk.get("residual_dense", False)), panes=panes[i])
        if b["kernel_size"] % 2 == 0:
            raise ValueError("block %d: kernel_size %d must be odd" % (i, b["kernel_size"]))
        if b["stride"] > 1 and b["dilation"] > 1:
            raise ValueError("block %d: only stride OR dilation may be greater than 1" % i)       # model.py:52-55
        if b["residual"] and b["stride"] != 1:
            raise ValueError("block %d: a residual block with stride %d is not built" % (i, b["stride"]))
        if b["repeat"] < 1:
            raise ValueError("block %d: repeat must be at least 1" % i)
        blocks.append(b)
        c = b["filters"]
    dec = cfg["jasper"].get("decoder") or {}
    if int(dec.get("in_feats", c)) != c:
        raise ValueError("decoder.in_feats %r does not match the encoder's %d output channels" % (dec.get("in_feats"), c))
    return labels, feats, blocks


def state_shapes(cfg):
    """name -> shape of Jasper(...).state_dict(), in its order."""
    labels, _, blocks = check_config(cfg)
    s = collections.OrderedDict()
    for n, b in enumerate(blocks):
        pre = "encoder.layers.%d." % n
        c = b["infilters"]
        for r in range(b["repeat"]):
            s["%sconv.%d.weight" % (pre, 4 * r)] = (b["filters"], c, b["kernel_size"])
            _bn_shapes(s, "%sconv.%d." % (pre, 4 * r + 1), b["filters"])
            c = b["filters"]
        for j, cj in enumerate(b["panes"]):
            s["%sres.%d.0.weight" % (pre, j)] = (b["filters"], cj, 1)
            _bn_shapes(s, "%sres.%d.1." % (pre, j), b["filters"])
    s["decoder.layers.0.weight"] = (len(labels) + 1, blocks[-1]["filters"], 1)
    s["decoder.layers.0.bias"] = (len(labels) + 1,)
    return s


V1_RULES = (("^jasper_encoder.encoder.", "encoder.layers."), ("^jasper_decoder.decoder_layers.", "decoder.layers."))


def convert_v1_state_dict(state):
    """common/helpers.py:168-183: the key names of the first release.  `acoustic_model.` and `audio_preprocessor.` entries are
    dropped, `jasper_encoder.encoder.` becomes `encoder.layers.` and `jasper_decoder.decoder_layers.` becomes `decoder.layers.`."""
    out = collections.OrderedDict()
    for k, v in state.items():
        if k.startswith("acoustic_model.") or k.startswith("audio_preprocessor."):
            continue
        for pattern, to in V1_RULES:
            k = re.sub(pattern, to, k)
        out[k] = v
    return out


class JasperModel(QuartzNetModel):
    """QuartzNetModel over Jasper's configuration and names; a state's keys of the first release are converted on the way in."""
    NAME = "Jasper"
    check_config, state_shapes = staticmethod(check_config), staticmethod(state_shapes)

    @staticmethod
    def normalize_keys(state):
        return convert_v1_state_dict(strip_module_prefix(state))
