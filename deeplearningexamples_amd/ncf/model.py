"""NeuMF, the host model of the NCF recipe (reference: PyTorch/Recommendation/NCF/neumf.py): the reference's parameter names
(mf_user_embed.weight, mf_item_embed.weight, mlp_user_embed.weight, mlp_item_embed.weight, mlp.<i>.weight / .bias, final.weight /
.bias), its initialisation, and its forward in torch operators -- the statement the GPU front end (infer.NeuMFScorer) is checked
against, and what a model.pth of the reference loads into.
"""
import math

import torch
import torch.nn as nn

from ..utils.state import strip_module_prefix

DEFAULT_FACTORS = 64
DEFAULT_LAYERS = (256, 256, 128, 64)


class NeuMFModel(nn.Module):
    def __init__(self, nb_users, nb_items, mf_dim=DEFAULT_FACTORS, mlp_layer_sizes=DEFAULT_LAYERS, dropout=0.0):
        layers = [int(n) for n in mlp_layer_sizes]
        if len(layers) < 2 or layers[0] % 2:
            raise ValueError("NeuMFModel: at least two MLP sizes and an even first one (got %s)" % (layers,))
        super().__init__()
        self.nb_users, self.nb_items, self.mf_dim, self.mlp_layer_sizes = int(nb_users), int(nb_items), int(mf_dim), tuple(layers)
        self.dropout = float(dropout)                 # evaluation only: kept for the command line, never applied
        self.mf_user_embed = nn.Embedding(self.nb_users, self.mf_dim)
        self.mf_item_embed = nn.Embedding(self.nb_items, self.mf_dim)
        self.mlp_user_embed = nn.Embedding(self.nb_users, layers[0] // 2)
        self.mlp_item_embed = nn.Embedding(self.nb_items, layers[0] // 2)
        self.mlp = nn.ModuleList(nn.Linear(layers[i - 1], layers[i]) for i in range(1, len(layers)))
        self.final = nn.Linear(layers[-1] + self.mf_dim, 1)
        with torch.no_grad():
            for emb in (self.mf_user_embed, self.mf_item_embed, self.mlp_user_embed, self.mlp_item_embed):
                emb.weight.normal_(0.0, 0.01)
            for lin in self.mlp:                      # glorot uniform
                limit = math.sqrt(6.0 / (lin.in_features + lin.out_features))
                lin.weight.uniform_(-limit, limit)
            limit = math.sqrt(3.0 / self.final.in_features)      # lecun uniform
            self.final.weight.uniform_(-limit, limit)

    def forward(self, user, item, sigmoid=False):
        xmf = self.mf_user_embed(user) * self.mf_item_embed(item)
        x = torch.cat((self.mlp_user_embed(user), self.mlp_item_embed(item)), dim=1)
        for lin in self.mlp:
            x = torch.relu(lin(x))
        x = self.final(torch.cat((xmf, x), dim=1))
        return torch.sigmoid(x) if sigmoid else x

    def load_state_dict(self, state, strict=True):
        return super().load_state_dict(strip_module_prefix(state), strict=strict)


def state_shapes(nb_users, nb_items, mf_dim=DEFAULT_FACTORS, mlp_layer_sizes=DEFAULT_LAYERS):
    """name -> shape, in the reference's state_dict order."""
    return {k: tuple(v.shape) for k, v in NeuMFModel(nb_users, nb_items, mf_dim, mlp_layer_sizes).state_dict().items()}


def model_from_state(state, dropout=0.0):
    """A NeuMFModel sized by a state dict (the reference's model.pth, with or without the `module.` prefix) and loaded from it."""
    state = strip_module_prefix(state)
    n_mlp = sum(1 for k in state if k.startswith("mlp.") and k.endswith(".weight"))
    layers = [state["mlp.0.weight"].shape[1]] + [state["mlp.%d.weight" % i].shape[0] for i in range(n_mlp)]
    m = NeuMFModel(state["mf_user_embed.weight"].shape[0], state["mf_item_embed.weight"].shape[0], state["mf_user_embed.weight"].shape[1],
                   layers, dropout)
    m.load_state_dict(state)
    return m.eval()


def load_checkpoint(path, dropout=0.0):
    """torch.load unpickles: load only files you trust."""
    return model_from_state(torch.load(path, map_location="cpu"), dropout)
