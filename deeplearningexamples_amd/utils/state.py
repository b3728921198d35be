"""Checkpoint-side helpers the model families share: key clean-up, the evaluation-mode BatchNorm fold, the YAML loader, and
ParamTable, the host model that is a table of tensors under the reference's names (no forward: that lives in the family's infer.py).
"""
import collections
import copy

import torch


def load_config(path_or_cfg):
    """The reference's YAML file (or the dict it holds) -> a deep copy as a dict."""
    if isinstance(path_or_cfg, dict):
        return copy.deepcopy(path_or_cfg)
    import yaml
    with open(path_or_cfg) as f:
        return yaml.safe_load(f)


def strip_module_prefix(state):
    """`module.` prefixes (DistributedDataParallel) stripped, the order kept."""
    out = collections.OrderedDict()
    for k, v in state.items():
        while k.startswith("module."):
            k = k[len("module."):]
        out[k] = v
    return out


def fold_bn(gamma, beta, running_mean, running_var, eps):
    """Evaluation-mode BatchNorm as y = scale * x + shift, in fp32: scale = gamma * rsqrt(running_var + eps),
    shift = beta - running_mean * scale."""
    scale = gamma.float() * torch.rsqrt(running_var.float() + eps)
    shift = beta.float() - running_mean.float() * scale
    return scale.contiguous(), shift.contiguous()


class ParamTable:
    """The parameters of `shapes` (name -> shape, in the reference's state_dict order) as fp32 tensors on `device`, zero until
    loaded; BatchNorm buffers as torch makes them: num_batches_tracked int64, running_var one.  A subclass sets NAME (what the
    messages call the state), may replace normalize_keys (applied to a state before it is compared with `shapes`) and may list in
    ABSENT_OK the key endings a state is allowed to lack."""
    NAME = None
    ABSENT_OK = ()
    normalize_keys = staticmethod(strip_module_prefix)

    def __init__(self, shapes, device):
        self.shapes, self.device = shapes, torch.device(device)
        self.params = collections.OrderedDict()
        for k, shape in shapes.items():
            if k.endswith("num_batches_tracked"):
                self.params[k] = torch.zeros(shape, dtype=torch.int64, device=self.device)
            elif k.endswith("running_var"):
                self.params[k] = torch.ones(shape, dtype=torch.float32, device=self.device)
            else:
                self.params[k] = torch.zeros(shape, dtype=torch.float32, device=self.device)

    def state_dict(self):
        return collections.OrderedDict(self.params)

    def load_state_dict(self, state):
        """Strict: every key of `shapes` (but ABSENT_OK), no other key, every shape as listed."""
        state = self.normalize_keys(state)
        want = self.shapes
        missing = [k for k in want if k not in state and not k.endswith(self.ABSENT_OK)]
        if missing:
            raise KeyError("%s state lacks %s" % (self.NAME, ", ".join(missing[:8])))
        for k, v in state.items():
            if k not in want:
                raise KeyError("unexpected key %r in a %s state" % (k, self.NAME))
            v = torch.as_tensor(v).detach().to(self.device, self.params[k].dtype)
            if tuple(v.shape) != tuple(want[k]):
                raise ValueError("%s: shape %s, expected %s" % (k, tuple(v.shape), tuple(want[k])))
            self.params[k] = v.clone()
        return self
