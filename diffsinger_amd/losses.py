"""DiffusionLoss, RectifiedFlowLoss and DurationLoss (modules/losses/) as device reductions: same constructors and
`forward` signatures, no backward pass.  Each returns a 0-dim fp32 tensor on the device, rounded once from the float64
mean that dsd_masked_loss / dsd_dur_score form (include/dsdenoise.h, "the rounding rule"): fp32 terms as the reference
forms them, summed in double in a fixed order - bit-identical from run to run.

`non_padding` is the tasks' `(mel2ph > 0).unsqueeze(-1).float()`, [B, T, 1] (or [B, T]): one value per frame.  A mask
that varies along the bins is not what any task passes and is refused.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from . import score


def _frame_mask(non_padding, pred):
    if non_padding is None:
        return None
    if non_padding.dim() == 3:
        if non_padding.shape[-1] != 1:
            raise ValueError(f"non_padding must be [B, T, 1] (one value per frame); got {tuple(non_padding.shape)}")
        non_padding = non_padding[..., 0]
    if tuple(non_padding.shape) != (pred.shape[0], pred.shape[-1]):
        raise ValueError(f"non_padding {tuple(non_padding.shape)} does not match the frames of {tuple(pred.shape)}")
    return non_padding


class _MaskedLoss(nn.Module):
    def __init__(self, loss_type):
        super().__init__()
        self.loss_type = loss_type
        if self.loss_type not in ('l1', 'l2'):
            raise NotImplementedError()

    def _reduce(self, pred, target, non_padding=None, t=None):
        out = score.masked_loss(self.loss_type, pred, target, _frame_mask(non_padding, pred), t)
        return out[1].to(torch.float32)


class DiffusionLoss(_MaskedLoss):
    """diff_loss.py:5-34"""

    def forward(self, x_recon: Tensor, noise: Tensor, non_padding: Tensor = None) -> Tensor:
        """
        :param x_recon: [B, 1, M, T]
        :param noise: [B, 1, M, T]
        :param non_padding: [B, T, 1]
        """
        return self._reduce(x_recon, noise, non_padding)


class RectifiedFlowLoss(_MaskedLoss):
    """reflow_loss.py:6-50"""

    def __init__(self, loss_type, log_norm=True):
        super().__init__(loss_type)
        self.log_norm = log_norm

    @staticmethod
    def get_weights(t):
        """The log-norm weights as the reference's fp32 torch ops give them (API parity; `forward` evaluates the same
        expression in double on the device)."""
        eps = 1e-7
        t = t.float()
        t = torch.clip(t, 0 + eps, 1 - eps)
        weights = 0.398942 / t / (1 - t) * torch.exp(
            -0.5 * torch.log(t / (1 - t)) ** 2
        ) + eps
        return weights[:, None, None, None]

    def forward(self, v_pred: Tensor, v_gt: Tensor, t: Tensor, non_padding: Tensor = None) -> Tensor:
        """
        :param v_pred: [B, 1, M, T]
        :param v_gt: [B, 1, M, T]
        :param t: [B,]
        :param non_padding: [B, T, 1]
        """
        return self._reduce(v_pred, v_gt, non_padding, t if self.log_norm else None)


class L1Loss(_MaskedLoss):
    """nn.L1Loss() of the aux decoders (aux_decoder/__init__.py:10-12): the mean of |input - target|, no mask."""

    def __init__(self):
        super().__init__('l1')

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        return self._reduce(input, target)


class DurationLoss(nn.Module):
    """
    Loss module as combination of phone duration loss, word duration loss and sentence duration loss (dur_loss.py:6-56).
    """

    def __init__(self, offset, loss_type,
                 lambda_pdur=0.6, lambda_wdur=0.3, lambda_sdur=0.1):
        super().__init__()
        self.loss_type = loss_type
        if self.loss_type not in ('mse', 'huber'):
            raise NotImplementedError()
        self.offset = offset

        self.lambda_pdur = lambda_pdur
        self.lambda_wdur = lambda_wdur
        self.lambda_sdur = lambda_sdur

    def linear2log(self, any_dur):
        return torch.log(any_dur + self.offset)

    def forward(self, dur_pred: Tensor, dur_gt: Tensor, ph2word: Tensor) -> Tensor:
        res = score.dur_score(dur_pred, dur_gt, ph2word, offset=self.offset, loss_type=self.loss_type)
        m = res["means"]        # float64: pdur + wdur + sdur in the reference's order, each mean weighted first
        return (self.lambda_pdur * m[0] + self.lambda_wdur * m[1] + self.lambda_sdur * m[2]).to(torch.float32)
