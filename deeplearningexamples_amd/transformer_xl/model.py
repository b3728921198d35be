"""Transformer-XL parameter container, vocabulary and checkpoint form (LanguageModeling/Transformer-XL/pytorch).

The reference's checkpoint (train.py:314-327) is a torch.save of {'args': argparse.Namespace, 'model_config': the keyword arguments
of MemTransformerLM, 'model_state': its state_dict(), 'vocab': a pickled utils.vocabulary.Vocab, ...}.  The reference's modules do
not exist here: `load_checkpoint` resolves `utils.vocabulary.Vocab` to this file's own `Vocab` while unpickling, and
`save_checkpoint` writes a file the reference's eval.py loads (the class is pickled under the reference's name).

Only the evaluation path of attn_type 0 (RelPartialLearnableMultiHeadAttn, post-LayerNorm) with the adaptive softmax is built;
`check_config` rejects the rest with one line each.
"""
import contextlib
import pickle
import sys
import types
from collections import OrderedDict

import torch


class Vocab:
    """utils/vocabulary.py:25-187, the part evaluation needs: tokenize / encode with a built symbol table."""

    def __init__(self, special=(), min_freq=0, max_size=None, lower_case=True, delimiter=None, vocab_file=None):
        self.special, self.min_freq, self.max_size = list(special), min_freq, max_size
        self.lower_case, self.delimiter, self.vocab_file = lower_case, delimiter, vocab_file
        self.idx2sym, self.sym2idx = [], OrderedDict()

    def add_special(self, sym):
        if sym not in self.sym2idx:
            self.add_symbol(sym)
            setattr(self, "%s_idx" % sym.strip("<>"), self.sym2idx[sym])

    def add_symbol(self, sym):
        if sym not in self.sym2idx:
            self.idx2sym.append(sym)
            self.sym2idx[sym] = len(self.idx2sym) - 1

    @classmethod
    def from_symbols(cls, symbols, special=("<eos>",), lower_case=False):
        v = cls(special=special, lower_case=lower_case)
        for s in special:
            v.add_special(s)
        for s in symbols:
            v.add_symbol(s)
        if "<unk>" in v.sym2idx:
            v.unk_idx = v.sym2idx["<unk>"]
        return v

    def tokenize(self, line, add_eos=False, add_double_eos=False):
        line = line.strip()
        if self.lower_case:
            line = line.lower()
        symbols = line if self.delimiter == "" else line.split(self.delimiter)
        symbols = list(symbols)
        if add_double_eos:
            return ["<S>"] + symbols + ["<S>"]
        return symbols + ["<eos>"] if add_eos else symbols

    def get_idx(self, sym):
        if sym in self.sym2idx:
            return self.sym2idx[sym]
        if "<eos>" in sym or not hasattr(self, "unk_idx"):
            raise KeyError("symbol %r is not in the vocabulary and it has no <unk>" % sym)
        return self.unk_idx

    def convert_to_tensor(self, symbols):
        return torch.tensor([self.get_idx(s) for s in symbols], dtype=torch.int64)

    def encode_file(self, path, ordered=True, add_eos=True):
        encoded = []
        with open(path, "r", encoding="utf-8") as f:
            for line in f:
                encoded.append(self.convert_to_tensor(self.tokenize(line, add_eos=add_eos)))
        if not ordered:
            return encoded
        return torch.cat(encoded) if encoded else torch.zeros(0, dtype=torch.int64)

    def __len__(self):
        return len(self.idx2sym)


class _OpaqueVocab:
    """Stands in for utils.vocabulary.OpenAIVocab: the checkpoint loads, evaluation with it is rejected."""


_REF_MODULE = "utils.vocabulary"


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module == _REF_MODULE:
            return Vocab if name == "Vocab" else _OpaqueVocab
        return super().find_class(module, name)


_PICKLE = types.SimpleNamespace(__name__="pickle", Unpickler=_Unpickler, load=lambda f, **kw: _Unpickler(f, **kw).load())


def load_checkpoint(path):
    """The dictionary the reference's train.py saved, on the CPU, with the vocabulary as this file's `Vocab`."""
    ckpt = torch.load(path, map_location="cpu", pickle_module=_PICKLE, weights_only=False)
    for key in ("model_config", "model_state"):
        if not isinstance(ckpt, dict) or key not in ckpt:
            raise KeyError("not a Transformer-XL checkpoint: no %r entry" % key)
    v = ckpt.get("vocab")
    if isinstance(v, Vocab) and "<unk>" in v.sym2idx and not hasattr(v, "unk_idx"):
        v.unk_idx = v.sym2idx["<unk>"]                                        # eval.py:353-354
    return ckpt


@contextlib.contextmanager
def _reference_names():
    """While a checkpoint is written `Vocab` answers to the reference's module path, so that the file names that class."""
    saved = {k: sys.modules.get(k) for k in ("utils", _REF_MODULE)}
    pkg, mod = types.ModuleType("utils"), types.ModuleType(_REF_MODULE)
    mod.Vocab, pkg.vocabulary = Vocab, mod
    own = Vocab.__module__
    sys.modules["utils"], sys.modules[_REF_MODULE], Vocab.__module__ = pkg, mod, _REF_MODULE
    try:
        yield
    finally:
        Vocab.__module__ = own
        for k, m in saved.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m


def save_checkpoint(path, model, vocab, args):
    """{'args', 'model_config', 'model_state', 'vocab'} as train.py:314-327 writes them (the training-only entries are left out:
    the reference's eval.py reads these four)."""
    state = {"args": args, "model_config": dict(model.cfg), "model_state": model.state_dict(), "vocab": vocab}
    with _reference_names():
        torch.save(state, path)


# ------------------------------------------------------------------------------------------------ configuration
CONFIG_KEYS = ("n_token", "n_layer", "n_head", "d_model", "d_head", "d_inner", "dropout", "dropatt", "dtype", "tie_weight",
               "d_embed", "div_val", "tie_projs", "pre_lnorm", "tgt_len", "ext_len", "mem_len", "cutoffs", "same_length",
               "attn_type", "clamp_len", "sample_softmax")


def check_config(cfg):
    """Keyword arguments of MemTransformerLM -> a normalised copy; what this package does not build is one line each."""
    cfg = dict(cfg)
    unknown = sorted(set(cfg) - set(CONFIG_KEYS))
    if unknown:
        raise ValueError("unknown model_config entries: %s" % ", ".join(unknown))
    for k in ("n_token", "n_layer", "n_head", "d_model", "d_head", "d_inner"):
        if k not in cfg:
            raise ValueError("model_config has no %r" % k)
    cfg.setdefault("d_embed", None)
    if cfg["d_embed"] is None:
        cfg["d_embed"] = cfg["d_model"]
    for k, d in (("dropout", 0.0), ("dropatt", 0.0), ("dtype", None), ("tie_weight", True), ("div_val", 1), ("tie_projs", [False]),
                 ("pre_lnorm", False), ("tgt_len", None), ("ext_len", 0), ("mem_len", 0), ("cutoffs", []), ("same_length", False),
                 ("attn_type", 0), ("clamp_len", -1), ("sample_softmax", -1)):
        cfg.setdefault(k, d)
    cfg["cutoffs"], cfg["tie_projs"] = list(cfg["cutoffs"]), list(cfg["tie_projs"])
    if cfg["attn_type"] != 0:
        raise ValueError("attn_type %r is not built: only 0 (relative positions with learnable biases)" % cfg["attn_type"])
    if cfg["pre_lnorm"]:
        raise ValueError("pre_lnorm is not built: LayerNorm follows the residual sum")
    if cfg["sample_softmax"] is not None and cfg["sample_softmax"] > 0:
        raise ValueError("sample_softmax > 0 is not built: the adaptive softmax only")
    if cfg["ext_len"]:
        raise ValueError("ext_len > 0 is not built")
    if cfg["d_head"] != 64:
        raise ValueError("d_head %r is not built: the attention kernel is written for 64-wide heads" % cfg["d_head"])
    ncl = len(cfg["cutoffs"]) + 1
    if len(cfg["tie_projs"]) < ncl:
        raise ValueError("tie_projs has %d entries for %d clusters" % (len(cfg["tie_projs"]), ncl))
    ends = [0] + cfg["cutoffs"] + [cfg["n_token"]]
    if any(b <= a for a, b in zip(ends, ends[1:])):
        raise ValueError("cutoffs must be increasing and below n_token")
    if cfg["d_model"] % 8 or cfg["d_inner"] % 8 or any((cfg["d_embed"] // cfg["div_val"] ** i) % 8 for i in range(ncl if cfg["div_val"] > 1 else 1)):
        raise ValueError("d_model, d_inner and every embedding width must be multiples of 8")
    return cfg


def state_shapes(cfg):
    """name -> shape, the names of MemTransformerLM(**cfg).state_dict() (tied entries under both of their names)."""
    n_token, d_model, d_embed, div_val = cfg["n_token"], cfg["d_model"], cfg["d_embed"], cfg["div_val"]
    h = cfg["n_head"] * cfg["d_head"]
    ends = [0] + list(cfg["cutoffs"]) + [n_token]
    ncl = len(ends) - 1
    widths = [d_embed // div_val ** i for i in range(ncl)]
    out = OrderedDict()
    if div_val == 1:
        out["word_emb.emb_layers.0.weight"] = (n_token, d_embed)
        if d_model != d_embed:
            out["word_emb.emb_projs.0"] = (d_model, d_embed)
    else:
        for i in range(ncl):
            out["word_emb.emb_layers.%d.weight" % i] = (ends[i + 1] - ends[i], widths[i])
        for i in range(ncl):
            out["word_emb.emb_projs.%d" % i] = (d_model, widths[i])
    for l in range(cfg["n_layer"]):
        p = "layers.%d." % l
        out[p + "dec_attn.qkv_net.weight"] = (3 * h, d_model)
        out[p + "dec_attn.o_net.weight"] = (d_model, h)
        out[p + "dec_attn.layer_norm.weight"] = (d_model,)
        out[p + "dec_attn.layer_norm.bias"] = (d_model,)
        out[p + "dec_attn.r_net.weight"] = (h, d_model)
        out[p + "pos_ff.CoreNet.0.weight"] = (cfg["d_inner"], d_model)
        out[p + "pos_ff.CoreNet.0.bias"] = (cfg["d_inner"],)
        out[p + "pos_ff.CoreNet.3.weight"] = (d_model, cfg["d_inner"])
        out[p + "pos_ff.CoreNet.3.bias"] = (d_model,)
        out[p + "pos_ff.layer_norm.weight"] = (d_model,)
        out[p + "pos_ff.layer_norm.bias"] = (d_model,)
    if ncl > 1:
        out["crit.cluster_weight"] = (ncl - 1, d_embed)
        out["crit.cluster_bias"] = (ncl - 1,)
    if div_val == 1:
        out["crit.out_layers_biases.0"] = (n_token,)
        if not cfg["tie_weight"]:
            out["crit.out_layers_weights.0"] = (n_token, d_embed)
        if d_model != d_embed:
            for i in range(ncl):
                if not cfg["tie_projs"][i]:
                    out["crit.out_projs.%d" % i] = (d_model, d_embed)
            out["crit.shared_out_projs.0"] = (d_model, d_embed)
    else:
        for i in range(ncl):
            out["crit.out_layers_biases.%d" % i] = (ends[i + 1] - ends[i],)
            if not cfg["tie_weight"]:
                out["crit.out_layers_weights.%d" % i] = (ends[i + 1] - ends[i], widths[i])
            if not cfg["tie_projs"][i]:
                out["crit.out_projs.%d" % i] = (d_model, widths[i])
            out["crit.shared_out_projs.%d" % i] = (d_model, widths[i])
    out["pos_emb.inv_freq"] = (d_model // 2,)
    out["r_w_bias"] = (cfg["n_head"], cfg["d_head"])
    out["r_r_bias"] = (cfg["n_head"], cfg["d_head"])
    return out


class TransformerXLModel:
    """The parameters of MemTransformerLM under the reference's names, fp32 on the host.  No forward here: infer.py runs it."""

    def __init__(self, config):
        self.cfg = check_config(config)
        self.shapes = state_shapes(self.cfg)
        self.params = OrderedDict()
        self.ends = [0] + self.cfg["cutoffs"] + [self.cfg["n_token"]]
        self.n_clusters = len(self.ends) - 1

    def load_state_dict(self, state):
        state = OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in state.items())
        missing = [k for k in self.shapes if k not in state and not k.startswith("crit.shared_out_projs.")
                   and k != "pos_emb.inv_freq"]
        extra = [k for k in state if k not in self.shapes]
        if missing or extra:
            raise KeyError("state dict does not match the configuration: missing %s, unexpected %s" % (missing[:4], extra[:4]))
        for k, shape in self.shapes.items():
            if k not in state:
                continue
            if tuple(state[k].shape) != tuple(shape):
                raise ValueError("%s: shape %s, the configuration needs %s" % (k, tuple(state[k].shape), tuple(shape)))
            self.params[k] = state[k].detach().to("cpu", torch.float32).contiguous()
        d = self.cfg["d_model"]
        self.params["pos_emb.inv_freq"] = 1.0 / (10000 ** (torch.arange(0.0, d, 2.0) / d))       # a buffer: a function of d_model
        for k in self.shapes:
            if k.startswith("crit.shared_out_projs."):
                self.params[k] = self.params["word_emb.emb_projs." + k.rsplit(".", 1)[1]]
        return self

    def state_dict(self):
        return OrderedDict((k, self.params[k]) for k in self.shapes)

    # ---- what the adaptive layers read (utils/proj_adaptive_softmax.py:147-167, get_out_proj :120-129)
    def out_weight(self, i):
        P, cfg = self.params, self.cfg
        if cfg["div_val"] == 1:
            w = P["word_emb.emb_layers.0.weight"] if cfg["tie_weight"] else P["crit.out_layers_weights.0"]
            return w[self.ends[i]:self.ends[i + 1]], P["crit.out_layers_biases.0"][self.ends[i]:self.ends[i + 1]]
        w = P["word_emb.emb_layers.%d.weight" % i] if cfg["tie_weight"] else P["crit.out_layers_weights.%d" % i]
        return w, P["crit.out_layers_biases.%d" % i]

    def out_proj(self, i):
        P, cfg = self.params, self.cfg
        if cfg["tie_projs"][i]:
            return P.get("word_emb.emb_projs.0") if cfg["div_val"] == 1 else P["word_emb.emb_projs.%d" % i]
        return P.get("crit.out_projs.%d" % i)

    @classmethod
    def from_checkpoint(cls, path_or_ckpt, **overrides):
        """-> (model, vocab, args).  overrides: tgt_len, ext_len, mem_len, clamp_len, same_length as eval.py:385-390 sets them."""
        ckpt = path_or_ckpt if isinstance(path_or_ckpt, dict) else load_checkpoint(path_or_ckpt)
        cfg = dict(ckpt["model_config"])
        cfg.update(overrides)
        cfg["dtype"] = None
        return cls(cfg).load_state_dict(ckpt["model_state"]), ckpt.get("vocab"), ckpt.get("args")
