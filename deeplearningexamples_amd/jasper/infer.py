"""Jasper inference on the gfx950 library: log-mel features -> log-probabilities / transcripts, the forward of
SpeechRecognition/Jasper/jasper/model.py:239-251 (Jasper.forward with use_conv_masks) behind the front end of
common/features.py and the leading pad of inference.py:329-333, in front of GreedyCTCDecoder and common/helpers.py's
ctc_decoder_predictions_tensor.

Layout.  Activations are 16-bit, channels-last and PACKED: [total_rows, C] with device int32 cu tables; there are no padding rows.
Every utterance is computed as the reference computes it at batch size 1: with masked convolutions that is what the reference gives
it in any batch, except that the reference also decodes the frames behind an utterance's length, which this does not copy.

Launches, for S sub-blocks in all and P residual panes in all (10x5dr: 53 and 1 + 2 + ... + 10 = 55):
  1   dle_qn_normalize_pack_lead     per-feature normalisation, mask, transpose, 16-bit cast, `pad_leading` zero rows in front
  S   dle_conv1d_bn_packed_fwd       dense conv + BatchNorm (+ the block's residual sum) + ReLU, one launch per sub-block
  P   dle_conv2d_fwd_affine          the residual panes of a block (1x1 conv + BatchNorm over [1, 1, rows, C]), computed FIRST and
                                     chained through the `residual` operand into a running sum, which the block's last sub-block
                                     consumes; every link of the chain is rounded to the storage type
  1   dle_gemm                       the decoder: fp32 logits [rows, 32] over the weight padded to 32 rows
  1   dle_ctc_greedy_packed          log_softmax, argmax, the CTC collapse
All block outputs of a dense run stay alive until the run ends.  The BatchNorm coefficients stay fp32 (utils.state.fold_bn);
the 16-bit weights are unmodified.

Host synchronisation.  The lengths are known on the host, so every cu table is built there and uploaded in ONE copy; the only
device-to-host read of a batch is the one that brings the tokens (or the log-probabilities) back.  `d2h_reads` counts them.

Not built (one-line errors): fp32, what model.check_config rejects, utterances of fewer than 2 frames (the reference's
normalisation gives NaN there).  No CPU path.

Everything but the weight packing of a block and the block loop is quartznet.infer.CTCRecognizer's.
"""
import torch

from .. import functional as F
from ..quartznet.infer import CTCRecognizer
from ..utils.frontend import require_16bit
from .model import JasperModel


class _Unit:
    __slots__ = ("w", "scale", "shift", "stride", "dilation")


class _Block:
    __slots__ = ("units", "panes", "dense")


class JasperRecognizer(CTCRecognizer):
    MODEL = JasperModel

    def __init__(self, model_or_state_dict, config=None, dtype=torch.float16, device=None, pad_leading=16):
        """As CTCRecognizer.  pad_leading: zero frames in front of every utterance's normalised features (inference.py
        --pad_leading).  The first release's key names are converted when a state dict is loaded (convert_v1_state_dict)."""
        require_16bit(dtype, type(self).__name__)              # here too: the dtype is rejected before pad_leading
        if int(pad_leading) < 0:
            raise ValueError("pad_leading must not be negative (got %r)" % (pad_leading,))
        self.pad_leading = int(pad_leading)
        super().__init__(model_or_state_dict, config, dtype, device)

    def _pack_block(self, n, b, P, bn):
        dev, dtype = self.dev, self.dtype
        pre = "encoder.layers.%d." % n
        blk = _Block()
        blk.units, blk.panes, blk.dense = [], [], b["dense"]
        for r in range(b["repeat"]):
            u = _Unit()
            u.stride, u.dilation = b["stride"], b["dilation"]
            u.w = F.pack_conv1d_weight(P["%sconv.%d.weight" % (pre, 4 * r)].float(), dtype).to(dev)
            u.scale, u.shift = bn("%sconv.%d." % (pre, 4 * r + 1))
            blk.units.append(u)
        for j in range(len(b["panes"])):
            w = P["%sres.%d.0.weight" % (pre, j)].float()[:, :, 0]
            blk.panes.append((w.to(dtype).contiguous().reshape(w.shape[0], 1, 1, w.shape[1]).to(dev),) +
                             bn("%sres.%d.1." % (pre, j)))
        return blk

    def _encode(self, x, lens):
        """x: fp32 [B, n_feat, max len] on the device -> (the packed encoder output, its row counts, its cu table)."""
        tabs, cu_all = self._tables(lens, self.pad_leading)
        ti, cu, total = 0, cu_all[0], sum(tabs[0])
        h = F.qn_normalize_pack_lead(x, cu, total, self.dtype, self.pad_leading)
        xs = [h]                                                           # the encoder's list (model.py:204-209)
        for blk in self.blocks:
            res = None
            for (w, s, sh), src in zip(blk.panes, xs):
                res = F.conv2d_fwd_affine(src.view(1, 1, total, src.shape[1]), w, s, sh,
                                          residual=None if res is None else res.view(1, 1, total, -1),
                                          relu=False).view(total, w.shape[0])
            h, last = xs[-1], len(blk.units) - 1
            for i, u in enumerate(blk.units):
                r = res if i == last else None
                if u.stride != 1:
                    ti += 1
                    cu_o, total_o = cu_all[ti], sum(tabs[ti])
                    h = F.conv1d_bn_packed_fwd(h, u.w, u.scale, u.shift, cu, cu_o, total_o, stride=u.stride,
                                               dilation=u.dilation, residual=r, relu=True)
                    cu, total = cu_o, total_o
                else:
                    h = F.conv1d_bn_packed_fwd(h, u.w, u.scale, u.shift, cu, stride=1, dilation=u.dilation, residual=r,
                                               relu=True)
            xs = xs + [h] if blk.dense else [h]
        return xs[-1], tabs[ti], cu
