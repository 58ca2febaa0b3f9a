"""RawCurveAccuracy, RawCurveR2Score, RhythmCorrectness and PhonemeDurationAccuracy (modules/metrics/) on the device:
the reference's `update(...)` / `compute()` / `reset()` and state names, as plain classes (no torchmetrics).  The states
accumulate on the device as int64 counts and float64 sums; one `update` is one dsd_curve_stats / dsd_dur_score call.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import score


class _Metric:
    """add_state / reset of torchmetrics.Metric, as far as these four use them; a state moves to the device of the first
    update."""

    def __init__(self, **kwargs):
        if kwargs:
            raise TypeError(f"unexpected arguments {sorted(kwargs)}: the torchmetrics options are not supported")
        self._defaults = {}

    def add_state(self, name, default, dist_reduce_fx=None):
        self._defaults[name] = default
        setattr(self, name, default.clone())

    def reset(self):
        for name, default in self._defaults.items():
            setattr(self, name, default.clone())

    def _add(self, name, value):
        setattr(self, name, getattr(self, name).to(value.device) + value)

    def __call__(self, *args, **kwargs):
        self.update(*args, **kwargs)
        return self.compute()


def _curve_checks(pred, target, mask):
    if mask is None:
        assert pred.shape == target.shape, f'shapes of pred and target mismatch: {pred.shape}, {target.shape}'
    else:
        assert pred.shape == target.shape == mask.shape, \
            f'shapes of pred, target and mask mismatch: {pred.shape}, {target.shape}, {mask.shape}'


class RawCurveAccuracy(_Metric):
    def __init__(self, *, tolerance, **kwargs):
        super().__init__(**kwargs)
        self.tolerance = tolerance
        self.add_state('close', default=torch.tensor(0, dtype=torch.int64), dist_reduce_fx='sum')
        self.add_state('total', default=torch.tensor(0, dtype=torch.int64), dist_reduce_fx='sum')

    def update(self, pred: Tensor, target: Tensor, mask=None) -> None:
        """

        :param pred: predicted curve
        :param target: reference curve
        :param mask: valid or non-padding mask
        """
        _curve_checks(pred, target, mask)
        counts, _ = score.curve_stats(pred, target, mask, self.tolerance)
        self._add('close', counts[0])
        self._add('total', counts[1])

    def compute(self) -> Tensor:
        return self.close / self.total


class RawCurveR2Score(_Metric):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.add_state('sum_squared_error', default=torch.tensor(0.0, dtype=torch.float64), dist_reduce_fx='sum')
        self.add_state('sum_error', default=torch.tensor(0.0, dtype=torch.float64), dist_reduce_fx='sum')
        self.add_state('residual', default=torch.tensor(0.0, dtype=torch.float64), dist_reduce_fx='sum')
        self.add_state('total', default=torch.tensor(0, dtype=torch.int64), dist_reduce_fx='sum')

    def update(self, pred: Tensor, target: Tensor, mask=None) -> None:
        """

        :param pred: predicted curve
        :param target: reference curve
        :param mask: valid or non-padding mask
        """
        _curve_checks(pred, target, mask)
        counts, sums = score.curve_stats(pred, target, mask)
        self._add('sum_squared_error', sums[1])
        self._add('sum_error', sums[0])
        self._add('residual', sums[2])
        self._add('total', counts[1])

    def compute(self) -> Tensor:
        return (1 - self.residual / (self.sum_squared_error - self.sum_error ** 2 / self.total)).to(torch.float32)


def linguistic_checks(pred, target, ph2word, mask=None):
    if mask is None:
        assert pred.shape == target.shape == ph2word.shape, \
            f'shapes of pred, target and ph2word mismatch: {pred.shape}, {target.shape}, {ph2word.shape}'
    else:
        assert pred.shape == target.shape == ph2word.shape == mask.shape, \
            f'shapes of pred, target and mask mismatch: {pred.shape}, {target.shape}, {ph2word.shape}, {mask.shape}'
    assert pred.ndim == 2, f'all inputs should be 2D, but got {pred.shape}'
    assert torch.any(ph2word > 0), 'empty word sequence'
    assert torch.all(ph2word >= 0), 'unexpected negative word index'
    assert ph2word.max() <= pred.shape[1], f'word index out of range: {ph2word.max()} > {pred.shape[1]}'
    assert torch.all(pred >= 0.), f'unexpected negative ph_dur prediction'
    assert torch.all(target >= 0.), f'unexpected negative ph_dur target'


class RhythmCorrectness(_Metric):
    def __init__(self, *, tolerance, **kwargs):
        super().__init__(**kwargs)
        assert 0. < tolerance < 1., 'tolerance should be within (0, 1)'
        self.tolerance = tolerance
        self.add_state('correct', default=torch.tensor(0, dtype=torch.int64), dist_reduce_fx='sum')
        self.add_state('total', default=torch.tensor(0, dtype=torch.int64), dist_reduce_fx='sum')

    def update(self, pdur_pred: Tensor, pdur_target: Tensor, ph2word: Tensor, mask=None) -> None:
        """

        :param pdur_pred: predicted ph_dur
        :param pdur_target: reference ph_dur
        :param ph2word: word division sequence
        :param mask: valid or non-padding mask
        """
        linguistic_checks(pdur_pred, pdur_target, ph2word, mask=mask)
        counts = score.dur_score(pdur_pred, pdur_target, ph2word, mask, rhythm_tolerance=self.tolerance)["counts"]
        self._add('correct', counts[0])
        self._add('total', counts[1])

    def compute(self) -> Tensor:
        return self.correct / self.total


class PhonemeDurationAccuracy(_Metric):
    def __init__(self, *, tolerance, **kwargs):
        super().__init__(**kwargs)
        self.tolerance = tolerance
        self.add_state('accurate', default=torch.tensor(0, dtype=torch.int64), dist_reduce_fx='sum')
        self.add_state('total', default=torch.tensor(0, dtype=torch.int64), dist_reduce_fx='sum')

    def update(self, pdur_pred: Tensor, pdur_target: Tensor, ph2word: Tensor, mask=None) -> None:
        """

        :param pdur_pred: predicted ph_dur
        :param pdur_target: reference ph_dur
        :param ph2word: word division sequence
        :param mask: valid or non-padding mask
        """
        linguistic_checks(pdur_pred, pdur_target, ph2word, mask=mask)
        counts = score.dur_score(pdur_pred, pdur_target, ph2word, mask, pdur_tolerance=self.tolerance)["counts"]
        self._add('accurate', counts[2])
        self._add('total', counts[3])

    def compute(self) -> Tensor:
        return self.accurate / self.total
