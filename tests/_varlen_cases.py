"""Shared cases of the packed (variable-length) attention tests: a padded batch whose valid rows ARE the packed rows.

padded S = 128 * ceil(max len / 128); every row of the padded batch -- padding included -- holds seeded finite values, so a result
that equals the padded kernel's at the valid rows is also shown to be independent of what the padding rows hold; the additive
mask is 0 on a sequence's first len keys and -10000 on the rest.
"""
import torch

from tests import _attention_reference as A

# (lengths, heads): heads = 2 throughout; 1, 3 and 16 heads on the 384 set
LENGTH_SETS = [[128], [1], [1, 31, 32, 33, 127, 128], [129, 200, 256, 5], [300, 384, 1, 257], [1024, 897, 3]]
CASES = [(ls, 2) for ls in LENGTH_SETS] + [([300, 384, 1, 257], nh) for nh in (1, 3, 16)]
SCALE = 0.125


def case_id(c):
    ls, nh = c
    return "L%s_h%d" % ("-".join(str(x) for x in ls), nh)


def padded_s(lengths):
    return A.BLK * ((max(lengths) + A.BLK - 1) // A.BLK)


def cu_seqlens(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + int(n))
    return torch.tensor(cu, dtype=torch.int32)


def valid_rows(lengths, s):
    """Flat row indices (into [B * s]) of the valid rows, in packed order."""
    return torch.cat([torch.arange(n, dtype=torch.int64) + b * s for b, n in enumerate(lengths)])


def build(lengths, nh, dtype, sigma=0.8, seed=11):
    """-> dict(s, qkv_pad [B s, 3H], mask_add [B, s], rows, qkv_packed [T, 3H], cu int32 [B + 1])."""
    s, b = padded_s(lengths), len(lengths)
    g = torch.Generator().manual_seed(seed + sum(lengths) + 7 * nh)
    qkv = (torch.randn(b * s, 3 * nh * A.D, generator=g) * sigma).to(dtype)
    lens = torch.tensor(lengths)
    mask_add = torch.where(torch.arange(s)[None, :] < lens[:, None], 0.0, A.NEG).float()
    rows = valid_rows(lengths, s)
    return dict(s=s, b=b, qkv_pad=qkv, mask_add=mask_add, rows=rows, qkv_packed=qkv[rows].contiguous(), cu=cu_seqlens(lengths))


def valid_mask(lengths, s, nh):
    """bool [B, nh, s, 1]: the valid query rows in the [b, nh, s, 64] layout of tests/_attention_reference."""
    lens = torch.tensor(lengths)
    return (torch.arange(s)[None, :] < lens[:, None])[:, None, :, None].expand(len(lengths), nh, s, 1)


def check_valid_rows(ctx_heads, case, lengths, nh, dtype, what):
    """check_generic (ik = 1, no keep mask) of a padded-layout ctx [b, nh, s, 64] at the valid rows: the float64 reference and the
    candidate are both zeroed at the padding rows, so a padding row contributes no error and no norm; the bars are the module's."""
    s, b = case["s"], case["b"]
    dctx = torch.zeros(b * s, nh * A.D, dtype=dtype)
    r = A.reference(case["qkv_pad"], dctx, case["mask_add"], None, b, s, nh, SCALE, 1.0)
    vm = valid_mask(lengths, s, nh)
    r = dict(r, ctx=torch.where(vm, r["ctx"], torch.zeros((), dtype=torch.float64)))
    got = torch.where(vm, ctx_heads.double(), torch.zeros((), dtype=torch.float64))
    return A.check_generic({"ctx": got}, r, dtype, what)
