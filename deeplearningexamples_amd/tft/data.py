"""Data side of the TFT recipe without pandas or scikit-learn: the reader of a preprocessed CSV split (what the reference's
data_utils.TFTDataset yields, data_utils.py:127-187), the q-risk metric (criterions.py:31-37) and the un-scaling of forecasts
(inference.py:34-69).  numpy and the csv module only.
"""
import csv
from collections import OrderedDict

import numpy as np
import torch

from .model import DataTypes, FeatureSpec, InputTypes

FEAT_NAMES = ("s_cat", "s_cont", "k_cat", "k_cont", "o_cat", "o_cont", "target", "id")
_SLOTS = ((InputTypes.STATIC, DataTypes.CATEGORICAL), (InputTypes.STATIC, DataTypes.CONTINUOUS), (InputTypes.KNOWN, DataTypes.CATEGORICAL),
          (InputTypes.KNOWN, DataTypes.CONTINUOUS), (InputTypes.OBSERVED, DataTypes.CATEGORICAL), (InputTypes.OBSERVED, DataTypes.CONTINUOUS),
          (InputTypes.TARGET, None), (InputTypes.ID, None))
DEFAULT_ID_COL = "id"


def _np_type(embed_type):
    if embed_type == DataTypes.CONTINUOUS:
        return np.float32
    if embed_type == DataTypes.CATEGORICAL:
        return np.int64
    raise ValueError("TFT data: only continuous and categorical columns are read (got %s)" % (embed_type,))


class TFTDataset:
    """Examples of `example_length` consecutive rows of one series, every `dataset_stride` rows, series in the order of their id.
    Item i is an OrderedDict over FEAT_NAMES of tensors [example_length, n_columns] (float32 / int64; an absent kind is an empty
    tensor), as the reference's dataset returns them."""

    def __init__(self, path, config):
        self.features = list(config.features)
        self.example_length, self.stride = int(config.example_length), int(config.dataset_stride)
        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        header, rows = rows[0][1:], [r[1:] for r in rows[1:] if r]               # the first column is the saved index
        time_col = next(f.name for f in self.features if f.feature_type == InputTypes.TIME)
        id_col = next(f.name for f in self.features if f.feature_type == InputTypes.ID)
        if id_col not in header:
            id_col = DEFAULT_ID_COL
            self.features = [f for f in self.features if f.feature_type != InputTypes.ID]
            self.features.append(FeatureSpec(DEFAULT_ID_COL, InputTypes.ID, DataTypes.CATEGORICAL))
        # one array per column name, of the type of the LAST feature that names it (the cast the reference's dictionary keeps)
        types = {f.name: _np_type(f.feature_embed_type) for f in self.features}
        raw = {name: np.asarray([float(r[header.index(name)]) for r in rows], dtype=np.float64) for name in types}
        order = np.argsort(raw[time_col], kind="stable")
        cols = {name: raw[name][order].astype(t) for name, t in types.items()}
        ids = cols[id_col]
        self.groups = []
        for key in np.unique(ids):
            sel = np.nonzero(ids == key)[0]
            if len(sel) >= self.example_length:
                self.groups.append({name: c[sel] for name, c in cols.items()})
        counts = [(len(g[id_col]) - self.example_length + 1) // self.stride for g in self.groups]
        self._cum = np.cumsum(counts) if counts else np.zeros(0, dtype=np.int64)

    def __len__(self):
        return int(self._cum[-1]) if len(self._cum) else 0

    def __getitem__(self, idx):
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        g = int(np.searchsorted(self._cum, idx, side="right"))
        e = idx - (int(self._cum[g - 1]) if g else 0)
        lo = e * self.stride
        group = self.groups[g]
        slots = [[] for _ in _SLOTS]
        for f in self.features:
            for s, (kind, embed) in enumerate(_SLOTS):
                if f.feature_type == kind and (embed is None or f.feature_embed_type == embed):
                    slots[s].append(torch.from_numpy(group[f.name][lo:lo + self.example_length].copy()))
        return OrderedDict((n, torch.stack(s, dim=-1) if s else torch.empty(0)) for n, s in zip(FEAT_NAMES, slots))


def batches(dataset, batch_size):
    """Consecutive examples stacked (the reference's DataLoader without shuffling); empty kinds stay empty tensors."""
    for lo in range(0, len(dataset), batch_size):
        items = [dataset[i] for i in range(lo, min(lo + batch_size, len(dataset)))]
        yield OrderedDict((n, torch.stack([it[n] for it in items]) if items[0][n].numel() else torch.empty(0)) for n in FEAT_NAMES)


def qrisk(pred, tgt, quantiles):
    """Normalised quantile loss per quantile: 2 mean(q max(t - p, 0) + (1 - q) max(p - t, 0)) / mean |t|; pred [N, steps, Q],
    tgt [N, steps, 1], quantiles [Q]."""
    pred, tgt, q = np.asarray(pred), np.asarray(tgt), np.asarray(quantiles)
    d = pred - tgt
    loss = (1 - q) * np.maximum(d, 0) + q * np.maximum(-d, 0)
    return (2 * loss.reshape(-1, loss.shape[-1]) / np.abs(tgt).mean()).mean(0)


def unscale(values, scaler):
    """values [N, steps] through scaler.inverse_transform, one step (column) at a time as the reference does."""
    values = np.asarray(values)
    out = np.empty(values.shape, dtype=np.float64)
    for j in range(values.shape[1]):
        out[:, j] = np.asarray(scaler.inverse_transform(values[:, j:j + 1]))[:, -1]
    return out


def unscale_per_id(values, ids, scalers):
    """Rows of one id go through that id's scaler.  Rows keep their order (the reference returns them grouped by id; its loader
    yields them in that order already)."""
    values, ids = np.asarray(values), np.asarray(ids).reshape(-1)
    out = np.empty(values.shape, dtype=np.float64)
    for key in np.unique(ids):
        sel = ids == key
        out[sel] = unscale(values[sel], scalers[key])
    return out
