"""Generator of G24 (tests/golden/g24_track.npz): the reference's own `cross_fade` and `save_wav`
(utils/infer_utils.py:89-104), driven by the loop of inference/ds_acoustic.py:231-259, on the layouts of tests/track_ref.py
(LAYOUTS and MALFORMED).  The waveforms come from seeds (track_ref.waveform) and are not stored; what is stored is the
layout (sample rate, offsets, lengths, seeds), the float64 track, the int16 samples `save_wav` wrote with norm off and on,
and - for the malformed layouts - the fact that the reference raised.  No reference text is stored.

Runs on a machine with the reference tree; the tests only read the .npz.  utils/infer_utils.py is loaded as a file of its
own (the package's __init__ pulls in the training stack), and librosa (imported there, never called on this path) is
stubbed when absent.

    python tests/golden/make_golden_track.py /path/to/reference
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import track_ref  # noqa: E402


def reference_fold(cross_fade, offsets, wavs, sample_rate):
    """The segment loop of ds_acoustic.py:231-259, `np.append` and all, with the reference's cross_fade."""
    result, current_length = np.zeros(0), 0
    for offset, waveform_pred in zip(offsets, wavs):
        silent_length = round(offset * sample_rate) - current_length
        if silent_length >= 0:
            result = np.append(result, np.zeros(silent_length))
            result = np.append(result, waveform_pred)
        else:
            result = cross_fade(result, waveform_pred, current_length + silent_length)
        current_length = current_length + silent_length + waveform_pred.shape[0]
    return result


def main(ref_root):
    try:
        import librosa  # noqa: F401
    except ImportError:
        sys.modules["librosa"] = types.ModuleType("librosa")
    from scipy.io import wavfile
    spec = importlib.util.spec_from_file_location("ref_infer_utils", os.path.join(ref_root, "utils", "infer_utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cross_fade, save_wav = ref.cross_fade, ref.save_wav
    out = {"names": np.array([c[0] for c in track_ref.LAYOUTS]), "bad_names": np.array([c[0] for c in track_ref.MALFORMED])}
    with tempfile.TemporaryDirectory() as tmp:
        for name, sr, offsets, lengths, seeds in track_ref.LAYOUTS:
            wavs = track_ref.layout_waves(lengths, seeds)
            track = reference_fold(cross_fade, offsets, wavs, sr)
            assert track.dtype == np.float64
            out[f"{name}_sr"] = np.array(sr)
            out[f"{name}_offsets"] = np.array(offsets, dtype=np.float64)
            out[f"{name}_lengths"] = np.array(lengths, dtype=np.int64)
            out[f"{name}_seeds"] = np.array(seeds, dtype=np.int64)
            out[f"{name}_track"] = track
            for norm in (False, True):
                path = os.path.join(tmp, "t.wav")
                save_wav(track.copy(), path, sr, norm=norm)             # save_wav scales its argument in place
                rate, data = wavfile.read(path)
                assert rate == sr and data.dtype == np.int16 and data.shape == track.shape
                out[f"{name}_pcm_norm" if norm else f"{name}_pcm"] = data
            print(f"{name}: sr {sr} starts {track_ref.starts_of(offsets, sr)} lengths {lengths} -> {track.shape[0]} samples, "
                  f"peak {np.abs(track).max():.6f}")
    for name, sr, offsets, lengths, seeds in track_ref.MALFORMED:
        try:
            reference_fold(cross_fade, offsets, track_ref.layout_waves(lengths, seeds), sr)
            raised = ""
        except ValueError as e:
            raised = type(e).__name__
        out[f"{name}_sr"] = np.array(sr)
        out[f"{name}_offsets"] = np.array(offsets, dtype=np.float64)
        out[f"{name}_lengths"] = np.array(lengths, dtype=np.int64)
        out[f"{name}_raised"] = np.array(raised)
        print(f"{name}: starts {track_ref.starts_of(offsets, sr)} lengths {lengths} -> reference raised {raised or 'nothing'}")
    path = os.path.join(HERE, "g24_track.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DSD_REFERENCE", "../reference"))
