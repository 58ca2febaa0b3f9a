"""Scoring a checkpoint on held-out data: the loss side of the reference's validation step on the device.

`AcousticScorer(model).losses(sample)` and `VarianceScorer(model).losses(sample)` are `run_model(sample, infer=False)` of
training/acoustic_task.py:119-169 and training/variance_task.py:162-249 - the same sample keys, the same hparams
(`lambda_aux_mel_loss`, `main_loss_type`, `main_loss_log_norm`, `lambda_dur_loss`, `lambda_pitch_loss`, `lambda_var_loss`,
`dur_prediction_args`) - on `forward_score` of the models and the loss modules of losses.py: one noising step and ONE
denoiser evaluation per predictor, no gradients.  Each loss is a 0-dim fp32 tensor on the device.

No dataset, logger or plotting code: a validation loop feeds collated batches (dicts of device tensors) and averages the
dicts it gets back, weighting by `sample['size']` as the reference does.  `build_metrics()` gives the task's metric objects
(metrics.py) under the reference's names; what they are updated with are `infer=True` predictions, which the models'
`forward` already produces.

Draws: by default torch's, in the reference's order.  `seed=` (an int, or B ints) makes every draw of a step on the device
from the items' seeds (noise.py), so that two checkpoints - or two precision modes - are scored on the same noise.
"""
from __future__ import annotations

import torch

from . import metrics
from .aux_decoder import build_aux_loss
from .hparams import hparams
from .losses import DiffusionLoss, DurationLoss, RectifiedFlowLoss
from .variance import VARIANCE_CHECKLIST


def _main_loss(diffusion_type):
    if diffusion_type == 'ddpm':
        return DiffusionLoss(loss_type=hparams['main_loss_type'])
    if diffusion_type == 'reflow':
        return RectifiedFlowLoss(loss_type=hparams['main_loss_type'], log_norm=hparams['main_loss_log_norm'])
    raise ValueError(f"Unknown diffusion type: {diffusion_type}")


def _apply_main(loss, diffusion_type, out, non_padding):
    if diffusion_type == 'ddpm':
        x_recon, noise = out
        return loss(x_recon, noise, non_padding=non_padding)
    v_pred, v_gt, t = out
    return loss(v_pred, v_gt, t=t, non_padding=non_padding)


def retake_masks(b, t, device):
    """[b, t] bool, the regions a training step asks the variance model to re-predict (variance_task.py:74-80): a
    whole item with probability 1/4, else one random span of frames [lo, hi) - half of the frames on average."""
    whole = torch.randint(0, 4, (b, 1), device=device) == 0
    ends = torch.randint(0, t + 1, (b, 2), device=device)
    lo, hi = ends.min(dim=1, keepdim=True).values, ends.max(dim=1, keepdim=True).values
    frame = torch.arange(t, device=device)[None]
    return whole | ((frame >= lo) & (frame < hi))


class AcousticScorer:
    """acoustic_task.py:104-169 for a `DiffSingerAcoustic` (or, with `sample['condition']`, an `AcousticDecoder`)."""

    def __init__(self, model):
        self.model = model
        self.diffusion_type = hparams['diffusion_type']
        assert self.diffusion_type in ['ddpm', 'reflow'], f"Unknown diffusion type: {self.diffusion_type}"
        self.use_shallow_diffusion = hparams['use_shallow_diffusion']
        if self.use_shallow_diffusion:
            self.aux_mel_loss = build_aux_loss(hparams['shallow_diffusion_args']['aux_decoder_arch'])
            self.lambda_aux_mel_loss = hparams['lambda_aux_mel_loss']
        self.mel_loss = _main_loss(self.diffusion_type)
        self.required_variances = [v for v in VARIANCE_CHECKLIST if hparams.get(f'use_{v}_embed', False)]

    def run_model(self, sample, **draws):
        """-> ShallowDiffusionOutput of forward_score.  draws: `t`, `noise`, `seed`."""
        target = sample['mel']              # [B, T_s, M]
        if 'condition' in sample:           # an AcousticDecoder: the encoder's output is given
            return self.model.forward_score(sample['condition'], target, **draws)
        variances = {name: sample[name] for name in self.required_variances}
        return self.model.forward_score(
            sample['tokens'], mel2ph=sample['mel2ph'], f0=sample['f0'], **variances, key_shift=sample.get('key_shift'),
            speed=sample.get('speed'), spk_embed_id=sample['spk_ids'] if hparams.get('use_spk_id') else None,
            languages=sample['languages'] if hparams.get('use_lang_id') else None, gt_mel=target, **draws)

    def losses(self, sample, **draws) -> dict:
        output = self.run_model(sample, **draws)
        losses = {}
        if output.aux_out is not None:
            norm_gt = self.model.aux_decoder.norm_spec(sample['mel'])
            losses['aux_mel_loss'] = self.lambda_aux_mel_loss * self.aux_mel_loss(output.aux_out, norm_gt)
        non_padding = (sample['mel2ph'] > 0).unsqueeze(-1).float()
        if output.diff_out is not None:
            losses['mel_loss'] = _apply_main(self.mel_loss, self.diffusion_type, output.diff_out, non_padding)
        return losses


class VarianceScorer:
    """variance_task.py:124-249 for a `DiffSingerVariance`."""

    def __init__(self, model):
        self.model = model
        self.diffusion_type = hparams['diffusion_type']
        self.use_spk_id = hparams['use_spk_id']
        self.use_lang_id = hparams['use_lang_id']
        self.predict_dur = hparams['predict_dur']
        if self.predict_dur:
            self.lambda_dur_loss = hparams['lambda_dur_loss']
            d = hparams['dur_prediction_args']
            self.dur_loss = DurationLoss(offset=d['log_offset'], loss_type=d['loss_type'], lambda_pdur=d['lambda_pdur_loss'],
                                         lambda_wdur=d['lambda_wdur_loss'], lambda_sdur=d['lambda_sdur_loss'])
        self.predict_pitch = hparams['predict_pitch']
        if self.predict_pitch:
            self.lambda_pitch_loss = hparams['lambda_pitch_loss']
            self.pitch_loss = _main_loss(self.diffusion_type)
        self.variance_prediction_list = [v for v in VARIANCE_CHECKLIST if hparams.get(f'predict_{v}', False)]
        self.predict_variances = len(self.variance_prediction_list) > 0
        self.lambda_var_loss = hparams['lambda_var_loss']
        if self.predict_variances:
            self.var_loss = _main_loss(self.diffusion_type)

    def build_metrics(self) -> dict:
        """The task's validation metrics under its names (variance_task.py:135-160)."""
        out = {}
        if self.predict_dur:
            out['rhythm_corr'] = metrics.RhythmCorrectness(tolerance=0.05)
            out['ph_dur_acc'] = metrics.PhonemeDurationAccuracy(tolerance=0.2)
        if self.predict_pitch:
            out['pitch_acc'] = metrics.RawCurveAccuracy(tolerance=0.5)
            out['pitch_r2'] = metrics.RawCurveR2Score()
        for name in self.variance_prediction_list:
            out[f'{name}_r2'] = metrics.RawCurveR2Score()
        return out

    def run_model(self, sample, *, pitch_retake=None, variance_retake=None, **draws):
        """-> (raw dur_pred, pitch forward_score output, variance forward_score output), each or None.  The retake
        masks default to random ones as in training (`retake_masks`); draws: `pitch_t`, `pitch_noise`, `variance_t`,
        `variance_noise`, `seed`."""
        mel2ph = sample.get('mel2ph')
        if self.predict_pitch or self.predict_variances:
            b, t = mel2ph.shape
            if self.predict_pitch and pitch_retake is None:
                pitch_retake = retake_masks(b, t, mel2ph.device)
            if self.predict_variances and variance_retake is None:
                variance_retake = {name: retake_masks(b, t, mel2ph.device) for name in self.variance_prediction_list}
        return self.model.forward_score(
            sample['tokens'], languages=sample['languages'] if self.use_lang_id else None, midi=sample.get('midi'),
            ph2word=sample.get('ph2word'), ph_dur=sample['ph_dur'], mel2ph=mel2ph, note_midi=sample.get('note_midi'),
            note_rest=sample.get('note_rest'), note_dur=sample.get('note_dur'), note_glide=sample.get('note_glide'),
            mel2note=sample.get('mel2note'), base_pitch=sample.get('base_pitch'), pitch=sample.get('pitch'),
            energy=sample.get('energy'), breathiness=sample.get('breathiness'), voicing=sample.get('voicing'),
            tension=sample.get('tension'), pitch_retake=pitch_retake, variance_retake=variance_retake,
            spk_id=sample['spk_ids'] if self.use_spk_id else None, **draws)

    def losses(self, sample, **draws) -> dict:
        dur_pred, pitch_pred, variances_pred = self.run_model(sample, **draws)
        losses = {}
        if dur_pred is not None:
            losses['dur_loss'] = self.lambda_dur_loss * self.dur_loss(dur_pred, sample['ph_dur'], ph2word=sample['ph2word'])
        mel2ph = sample.get('mel2ph')
        non_padding = (mel2ph > 0).unsqueeze(-1) if mel2ph is not None else None
        if pitch_pred is not None:
            losses['pitch_loss'] = self.lambda_pitch_loss * _apply_main(self.pitch_loss, self.diffusion_type, pitch_pred,
                                                                        non_padding)
        if variances_pred is not None:
            losses['var_loss'] = self.lambda_var_loss * _apply_main(self.var_loss, self.diffusion_type, variances_pred,
                                                                    non_padding)
        return losses
