"""Dice as the reference counts it (nnunet/metrics.py, the --brats branch: compute_stats_brats), on whatever device the tensors are."""
import torch


def compute_stats_brats(logits, label):
    """logits [N, 3, D, H, W], label [N, D, H, W] with classes 0..3 -> Dice per channel, fp32 [3], over the whole batch.  The three
    channels are the BraTS regions -- whole tumour (label > 0), tumour core (label 1 or 3), enhancing tumour (label 3) -- and a voxel
    is predicted where sigmoid(logit) > 0.5.  Dice = 2 TP / (2 TP + FP + FN); a region without any target voxel scores 1 when nothing
    is predicted for it and 0 otherwise.  The reference stores channel i in slot i - 1 (metrics.py:48,53), so the vector reads
    (tumour core, enhancing tumour, whole tumour); the mean, which it reports as "Dice", does not depend on that."""
    pred = torch.sigmoid(logits) > 0.5
    target = torch.stack((label > 0, (label == 1) | (label == 3), label == 3), dim=1)
    over = [0] + list(range(2, pred.dim()))
    count = lambda t: t.sum(dim=over)
    tp, fp, fn = count(pred & target), count(pred & ~target), count(~pred & target)
    dice = (2 * tp).float() / (2 * tp + fp + fn).clamp(min=1).float()
    nothing_predicted = (count(pred) == 0).float()
    per_channel = torch.where(count(target) == 0, nothing_predicted, dice)
    return torch.roll(per_channel, -1)


class Dice:
    """Running mean over update() calls, in percent (Dice.compute)."""

    def __init__(self, n_class=3):
        self.n_class, self.steps, self.dice = n_class, 0, None

    def update(self, p, y):
        s = compute_stats_brats(p, y)
        self.dice = s if self.dice is None else self.dice + s
        self.steps += 1

    def compute(self):
        if not self.steps:
            raise ValueError("Dice.compute: no update() yet")
        return 100 * self.dice / self.steps
