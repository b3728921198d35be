"""QuartzNet's parameters under the reference's names (SpeechRecognition/QuartzNet/quartznet/model.py:115-357: JasperBlock,
JasperEncoder, JasperDecoderForCTC, QuartzNet) and its configuration as the reference's YAML holds it
(configs/quartznet15x5_speedp-online-1.15_speca.yaml: `labels`, `input_val.filterbank_features`, `quartznet.encoder`,
`quartznet.decoder`).

A container, not a module: it holds the tensors of `QuartzNet(encoder_kw, decoder_kw).state_dict()` --
  encoder.layers.N.mconv.M.*  a separable unit r of block N is mconv.{5r} (depthwise conv.weight [C, 1, K]), mconv.{5r + 1} (pointwise
                              conv.weight [Ko, C, 1]), mconv.{5r + 2} (BatchNorm1d: weight, bias, running_mean, running_var,
                              num_batches_tracked); 5r + 3 / 5r + 4 are the activation and the dropout (no tensors, absent behind the
                              last unit); a unit that is not separable is mconv.{4r} (conv), mconv.{4r + 1} (BatchNorm1d);
  encoder.layers.N.res.0.0.weight [Ko, C, 1], encoder.layers.N.res.0.1.*   the residual branch (1x1 conv, BatchNorm1d);
  decoder.layers.0.weight [n_classes, C, 1], decoder.layers.0.bias
-- and has no forward: that lives in quartznet/infer.py.
"""
import collections

from ..utils.state import ParamTable, load_config

BN_EPS = 1e-3                  # model.py:240
BLOCK_KEYS = ("filters", "repeat", "kernel_size", "kernel_size_factor", "stride", "dilation", "padding", "dropout", "residual",
              "residual_dense", "groups", "separable", "heads", "normalization", "norm_groups")


def apply_overrides(cfg, overrides):
    """--override_config KEY=VALUE (quartznet/config.py:122-140): dotted keys into the nested dict, the value parsed as YAML, so
    `false` and `False` both give a boolean.  The sections must exist; the last field may be new, as in the reference."""
    import yaml
    for item in overrides or ():
        if "=" not in item:
            raise ValueError("--override_config %r: expected KEY=VALUE" % (item,))
        key, val = item.split("=", 1)
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            if not isinstance(node, dict) or p not in node:
                raise ValueError("--override_config %s: no such key" % key)
            node = node[p]
        if not isinstance(node, dict):
            raise ValueError("--override_config %s: no such key" % key)
        node[parts[-1]] = yaml.safe_load(val)
    return cfg


def _one(v, what):
    if isinstance(v, (list, tuple)):
        if len(v) != 1:
            raise ValueError("%s must hold one value (got %r)" % (what, v))
        v = v[0]
    return int(v)


def check_config(cfg):
    """What inference builds of a QuartzNet YAML -> (labels, features dict, list of block dicts with plain ints).  Everything else
    is rejected with a one-line message."""
    if "quartznet" not in cfg or "encoder" not in cfg["quartznet"]:
        raise ValueError("not a QuartzNet config: no quartznet.encoder section")
    enc = cfg["quartznet"]["encoder"]
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
    blocks = []
    c = int(enc["in_feats"])
    for i, blk in enumerate(enc.get("blocks") or []):
        for k in blk:
            if k not in BLOCK_KEYS:
                raise ValueError("block %d: unknown key %r" % (i, k))
        if blk.get("normalization", "batch") != "batch":
            raise ValueError("block %d: normalization %r: only batch is built" % (i, blk.get("normalization")))
        if int(blk.get("groups", 1)) != 1:
            raise ValueError("block %d: groups %r: only 1 is built" % (i, blk.get("groups")))
        if blk.get("residual_dense", False):
            raise ValueError("block %d: residual_dense: dense residuals (Jasper) are not built" % i)
        if blk.get("padding", "same") not in ("same", ["same"]):
            raise ValueError("block %d: only 'same' padding is built" % i)
        if float(blk.get("kernel_size_factor", 1)) != 1.0:
            raise ValueError("block %d: kernel_size_factor %r: only 1 is built" % (i, blk.get("kernel_size_factor")))
        if int(blk.get("heads", -1)) != -1:
            raise ValueError("block %d: heads are not built" % i)
        b = dict(infilters=c, filters=int(blk["filters"]), repeat=int(blk.get("repeat", 3)),
                 kernel_size=_one(blk.get("kernel_size", 11), "kernel_size"), stride=_one(blk.get("stride", 1), "stride"),
                 dilation=_one(blk.get("dilation", 1), "dilation"), residual=bool(blk.get("residual", True)),
                 separable=bool(blk.get("separable", False)))
        if b["kernel_size"] % 2 == 0:
            raise ValueError("block %d: kernel_size %d must be odd" % (i, b["kernel_size"]))
        if b["stride"] > 1 and b["dilation"] > 1:
            raise ValueError("block %d: only stride OR dilation may be greater than 1" % i)       # model.py:60-63
        if b["residual"] and b["stride"] != 1:
            raise ValueError("block %d: a residual block with stride %d is not built" % (i, b["stride"]))
        if b["repeat"] < 1:
            raise ValueError("block %d: repeat must be at least 1" % i)
        blocks.append(b)
        c = b["filters"]
    if not blocks:
        raise ValueError("the encoder has no blocks")
    dec = cfg["quartznet"].get("decoder") or {}
    if int(dec.get("in_feats", c)) != c:
        raise ValueError("decoder.in_feats %r does not match the encoder's %d output channels" % (dec.get("in_feats"), c))
    return labels, feats, blocks


def _bn_shapes(s, p, c):
    s[p + "weight"] = (c,)
    s[p + "bias"] = (c,)
    s[p + "running_mean"] = (c,)
    s[p + "running_var"] = (c,)
    s[p + "num_batches_tracked"] = ()


def state_shapes(cfg):
    """name -> shape of QuartzNet(...).state_dict(), in its order."""
    labels, _, blocks = check_config(cfg)
    s = collections.OrderedDict()
    for n, b in enumerate(blocks):
        pre = "encoder.layers.%d." % n
        c = b["infilters"]
        m = 0
        for r in range(b["repeat"]):
            if b["separable"]:
                s["%smconv.%d.weight" % (pre, m)] = (c, 1, b["kernel_size"])
                s["%smconv.%d.weight" % (pre, m + 1)] = (b["filters"], c, 1)
                _bn_shapes(s, "%smconv.%d." % (pre, m + 2), b["filters"])
                m += 5
            else:
                s["%smconv.%d.weight" % (pre, m)] = (b["filters"], c, b["kernel_size"])
                _bn_shapes(s, "%smconv.%d." % (pre, m + 1), b["filters"])
                m += 4
            c = b["filters"]
        if b["residual"]:
            s[pre + "res.0.0.weight"] = (b["filters"], b["infilters"], 1)
            _bn_shapes(s, pre + "res.0.1.", b["filters"])
    s["decoder.layers.0.weight"] = (len(labels) + 1, blocks[-1]["filters"], 1)
    s["decoder.layers.0.bias"] = (len(labels) + 1,)
    return s


class QuartzNetModel(ParamTable):
    """The parameters as fp32 tensors (num_batches_tracked int64) on `device`, zero until loaded (running_var one).  A subclass
    for another network of the family replaces NAME, check_config, state_shapes and normalize_keys."""
    NAME = "QuartzNet"
    ABSENT_OK = ("num_batches_tracked",)
    check_config, state_shapes = staticmethod(check_config), staticmethod(state_shapes)

    def __init__(self, cfg, device="cpu"):
        self.cfg = load_config(cfg)
        self.labels, self.features, self.blocks = self.check_config(self.cfg)
        super().__init__(self.state_shapes(self.cfg), device)
