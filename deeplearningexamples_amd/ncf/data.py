"""The NCF test set (reference: PyTorch/Recommendation/NCF/feature_spec.py, dataloading.py:37-173): the feature specification
YAML, the torch_tensor chunk files, and the test loader for one device -- the de-duplication sort, the duplicate mask that never
hides the label-1 copy of an item, and the split into --valid_batch_size batches.  World size 1 only.
"""
import os

import torch

USER_CHANNEL, ITEM_CHANNEL, LABEL_CHANNEL = "user_ch", "item_ch", "label_ch"
TEST_SAMPLES_PER_SERIES = "test_samples_per_series"


class FeatureSpec:
    def __init__(self, feature_spec, source_spec, channel_spec, metadata, base_directory):
        self.feature_spec, self.source_spec, self.channel_spec = feature_spec, source_spec, channel_spec
        self.metadata, self.base_directory = metadata, base_directory
        for ch in (USER_CHANNEL, ITEM_CHANNEL, LABEL_CHANNEL):
            if len(channel_spec.get(ch, ())) != 1:
                raise ValueError("feature spec: channel %s must name exactly one feature" % ch)

    @classmethod
    def from_yaml(cls, path):
        import yaml
        with open(path) as f:
            d = yaml.safe_load(f)
        return cls(base_directory=os.path.dirname(path), **d)

    def name(self, channel):
        return self.channel_spec[channel][0]

    def cardinality(self, channel):
        return int(self.feature_spec[self.name(channel)]["cardinality"])


def load_features(spec, mapping, device="cpu"):
    """feature name -> [N, 1] tensor, from the chunks of source_spec[mapping] (one torch_tensor file per chunk, one column per
    feature).  torch.load unpickles: load only files you trust."""
    features = {}
    for chunk in spec.source_spec[mapping]:
        if chunk["type"] != "torch_tensor":
            raise ValueError("only torch_tensor chunks are read (got %r)" % chunk["type"])
        if len(chunk["files"]) != 1:
            raise ValueError("one file per chunk (got %d)" % len(chunk["files"]))
        data = torch.load(os.path.join(spec.base_directory, chunk["files"][0]), map_location=device)
        for col, name in enumerate(chunk["features"]):
            features[name] = data[:, col:col + 1].reshape(-1, 1)
    return features


class TestLoader:
    """users / items / labels / mask as flat tensors in the loader's order, and `batches`: a list of (user, item, label) views of
    at most valid_batch_size elements.  raw_length is the number of test samples, samples_in_series the metadata entry."""
    __test__ = False

    def __init__(self, spec, features, valid_batch_size, world_size=1):
        if world_size != 1:
            raise SystemExit("distributed evaluation is not built: run with WORLD_SIZE unset or 1 (got %d)" % world_size)
        S = self.samples_in_series = int(spec.metadata[TEST_SAMPLES_PER_SERIES])
        users, items, labels = (features[spec.name(c)] for c in (USER_CHANNEL, ITEM_CHANNEL, LABEL_CHANNEL))
        self.raw_length = users.shape[0]
        if items.shape[0] != self.raw_length or labels.shape[0] != self.raw_length or self.raw_length % S:
            raise ValueError("test set: %d users, %d items, %d labels are not whole series of %d" %
                             (users.shape[0], items.shape[0], labels.shape[0], S))
        users, items, labels = users.view(-1, S), items.view(-1, S), labels.view(-1, S)
        # Items ascending, the label-1 copy of an item in front of its label-0 copies: a duplicate is then an element equal to
        # its left neighbour, and the positive is never one.
        order = torch.sort(items.float() - labels.float() * 0.5)[1]
        items, labels, users = torch.gather(items, 1, order), torch.gather(labels, 1, order), torch.gather(users, 1, order)
        dup = items[:, :-1] == items[:, 1:]
        dup = torch.cat((torch.zeros_like(dup[:, :1]), dup), dim=1)
        self.users, self.items, self.labels, self.mask = users.reshape(-1), items.reshape(-1), labels.reshape(-1), dup.reshape(-1)
        self.batch_size = int(valid_batch_size)
        self.batches = list(zip(self.users.split(self.batch_size), self.items.split(self.batch_size), self.labels.split(self.batch_size)))

    def to(self, device):
        self.users, self.items, self.labels, self.mask = (t.to(device) for t in (self.users, self.items, self.labels, self.mask))
        self.batches = list(zip(self.users.split(self.batch_size), self.items.split(self.batch_size), self.labels.split(self.batch_size)))
        return self
