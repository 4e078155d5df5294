"""
The block-online beamformer as float64 numpy, from the operators of oracle/np_oracle.py: what
setk_enhance_online_batch (include/setk_hip.h) and the per-utterance loop of
apply_adaptive_beamformer.py --online.chunk-size are held to.

Per utterance, chunk c over the frames [c S, min((c + 1) S, T)):
    rs_c, rn_c   compute_covar over the chunk's frames alone (mask_s; mask_n or 1 - mask_s)
    Rs_c = alpha Rs_{c-1} + phi_c rs_c, Rn_c likewise, Rs_{-1} = 0
    phi_0 = 1, phi_c = 1 - alpha afterwards          (reference_phi: phi_c = 1 for every chunk, what
                                                      the reference class computes because it never
                                                      clears its `reset` member, libs/beamformer.py:296-317)
    w_c          mvdr_weight / gevd_weight(Rs_c, Rn_c); with ban do_ban(w_c, rn_c): the chunk's own
                 unsmoothed noise covariance
    frame t      beamformed with w_{t // S}
then the optional post-mask, one inverse_stft over the utterance and the renorm, as offline.

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***
"""
import numpy as np

from oracle import np_oracle as o

STFT_KW = dict(frame_len=512, frame_hop=256, window="hann", center=True)


def weight_of(kind, Rs, Rn, gauge=True):
    if kind == "mvdr":
        return o.mvdr_weight(Rs, Rn, gauge=gauge)
    if kind == "gevd":
        return o.gevd_weight(Rs, Rn, gauge=gauge)
    raise ValueError(kind)


def online_parts(obs, mask_s, chunk_size, alpha, kind="mvdr", mask_n=None, ban=False, gauge=True,
                 reference_phi=False, promote=True):
    """obs N x F x T complex, masks T x F.  Returns dict(Rs, Rn [chunks][F][N][N], rn (the chunks'
    own), weight [chunks][F][N] (after BAN), enh F x T).  promote=False leaves the observations
    and masks in the precision they come in, as the reference does with a complex64 spectrogram:
    its chunk covariances are then complex64 sums and only the smoothed state is complex128."""
    if promote:
        obs = np.asarray(obs, dtype=np.complex128)
        mask_s = np.asarray(mask_s, dtype=np.float64)
        mask_n = None if mask_n is None else np.asarray(mask_n, dtype=np.float64)
    mask_n = 1 - mask_s if mask_n is None else mask_n
    N, F, T = obs.shape
    Rs, Rn = np.zeros((F, N, N), dtype=np.complex128), np.zeros((F, N, N), dtype=np.complex128)
    out = dict(Rs=[], Rn=[], rn=[], weight=[])
    enh = np.empty((F, T), dtype=np.complex128)
    for c, t0 in enumerate(range(0, T, chunk_size)):
        sl = slice(t0, min(t0 + chunk_size, T))
        rn = o.compute_covar(obs[:, :, sl], mask_n[sl])
        rs = o.compute_covar(obs[:, :, sl], mask_s[sl])
        phi = 1.0 if (c == 0 or reference_phi) else 1.0 - alpha
        Rs = alpha * Rs + phi * rs
        Rn = alpha * Rn + phi * rn
        w = weight_of(kind, Rs, Rn, gauge=gauge)
        if ban:
            w = o.do_ban(w, rn)
        enh[:, sl] = o.beamform(w, obs[:, :, sl])
        for key, value in (("Rs", Rs), ("Rn", Rn), ("rn", rn), ("weight", w)):
            out[key].append(value)
    out = {key: np.stack(value) for key, value in out.items()}
    out["enh"] = enh
    return out


def weights_on(kind, Rs, Rn):
    """The weights of given covariance stacks [chunks][F][N][N] (e.g. the device's tapped float32
    matrices) in complex128, under the gauge."""
    return np.stack([weight_of(kind, np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128))
                     for a, b in zip(Rs, Rn)])


def enhance_online(samps, mask, chunk_size, alpha=0.8, kind="mvdr", itf_mask=None, ban=False, post_mask=False,
                   vad_proportion=1, gauge=True, reference_phi=False, promote=True, return_parts=False):
    """The body of run_online (apply_adaptive_beamformer.py) for one utterance: samps C x N float32,
    mask T x F (or F x T) -> the float waveform, renormed to max |samps|."""
    kw = dict(transpose=False, **STFT_KW)
    obs = o.multichannel_stft(samps, round_power_of_two=True, **kw)
    F = obs.shape[1]
    speech = np.asarray(mask)
    itf = None if itf_mask is None else np.asarray(itf_mask)
    if itf is None:
        speech = np.minimum(speech, 1)
    if speech.shape[0] == F and speech.shape[1] != F:
        speech = speech.T
        itf = None if itf is None else itf.T
    if 0.5 < vad_proportion < 1:
        vad, _ = o.compute_vad_masks(obs[0], vad_proportion)
        speech = np.where(vad, 1.0e-4, speech)
        itf = None if itf is None else np.where(vad, 1.0e-4, itf)
    parts = online_parts(obs, speech, chunk_size, alpha, kind=kind, mask_n=itf, ban=ban, gauge=gauge,
                         reference_phi=reference_phi, promote=promote)
    enh = parts["enh"]
    if post_mask:
        enh = enh * speech.T
    wav = o.inverse_stft(enh, norm=float(np.max(np.abs(samps))), **kw)
    if return_parts:
        parts.update(obs=obs, enh_out=enh)
        return wav, parts
    return wav


def case_inputs(C, N, index=None):
    """The inputs of the online tests: o.synth_utterance(30 + C, C, N) and the mask 0.05 + 0.9 irm."""
    mix, sp, nz = o.synth_utterance((30 + C) if index is None else index, C, N, return_parts=True)
    return mix, (0.05 + 0.9 * o.irm_mask(sp, nz)).astype(np.float32)
