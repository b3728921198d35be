"""HR@K, NDCG@K and the validation loss of one pass over the test set (reference: val_epoch, PyTorch/Recommendation/NCF/ncf.py:
128-178) on NeuMFScorer and dle_ncf_rank_fwd.

Per batch: one score launch (probabilities straight into the ratings vector, the loss partials beside it) and one rank launch over
the series the batch completed -- a series may straddle two batches, --valid_batch_size need not be a multiple of the series
length.  hits, dcg and the per-batch mean losses are summed on the device; three numbers are read once, at the end.
"""
import torch

from .. import functional as F


def evaluate(scorer, loader, k):
    """-> (hr, ndcg, validation_loss) as Python floats: hits / series, dcg / series, and the mean over the batches of each batch's
    mean binary cross-entropy, as val_epoch computes it."""
    S, n = loader.samples_in_series, loader.raw_length
    if not 1 <= k <= S:
        raise SystemExit("--topk %d does not fit a series of %d samples: the top k of fewer than k elements is undefined" % (k, S))
    dev = scorer.dev
    ratings = torch.empty(n, dtype=torch.float32, device=dev)
    labels = loader.labels.to(device=dev, dtype=torch.float32)
    mask = loader.mask.to(dev)
    totals = torch.zeros(3, dtype=torch.float64, device=dev)          # hits, dcg, sum of the batches' mean losses
    done, ranked = 0, 0                                               # samples scored, series ranked
    for user, item, label in loader.batches:
        b = user.numel()
        _, loss = scorer.score_with_loss(user, item, labels[done:done + b], prob_out=ratings[done:done + b])
        totals[2] += loss / b
        done += b
        whole = done // S
        if whole > ranked:
            lo, hi = ranked * S, whole * S
            hits, dcg = F.ncf_rank_fwd(ratings[lo:hi], labels[lo:hi], mask[lo:hi], S, k)
            totals[0] += hits.sum()
            totals[1] += dcg.sum(dtype=torch.float64)
            ranked = whole
    hits, dcg, loss = totals.cpu().tolist()                           # the evaluation's one host read
    series = n / S
    return hits / series, dcg / series, loss / max(len(loader.batches), 1)
