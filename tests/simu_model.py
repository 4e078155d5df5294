"""
*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE ***

A float64 restatement of the reference's scripts/sptk/wav_simulate.py (run_simu and its helpers,
:17-312) on arrays instead of files, the table of fixture cases, and a float32 emulation of the
partitioned overlap-save convolution the device runs (csrc/simu.hip), so that the kernel's
expected rounding is stated where a CPU can run it.

A case is a dict of arrays and options (see CASES / make_case); audio is int16 as a wave file
stores it and enters every computation as int16 / 32768 (read_wav).
"""
import numpy as np

EPSILON = float(np.finfo(np.float32).eps)
B = 256


def pcm_to_float(x):
    return np.asarray(x, dtype=np.float32) / np.float32(32768.0)


def coeff_snr(sig_pow, ref_pow, snr):
    return (ref_pow / (sig_pow * 10**(snr / 10) + EPSILON))**0.5


def convolve64(spk, rir):
    """ss.convolve(spk[None], rir)[..., :S] in float64, directly."""
    spk = np.asarray(spk, dtype=np.float64)
    rir = np.atleast_2d(np.asarray(rir, dtype=np.float64))
    return np.stack([np.convolve(spk, h)[:spk.size] for h in rir])


def partitioned32(spk, rir):
    """The device's scheme in float32: RIR blocks of 256 zero-padded to 512, source frames
    [(k-1) B, (k+1) B) with zeros in front, Y[k] = sum_p X[k-p] H[p] accumulated in order of p,
    the last 256 samples of every inverse transform.  (scipy.fft keeps float32; the device's own
    butterflies round differently by a few ulp, the scheme is the same.)"""
    import scipy.fft
    spk = np.asarray(spk, dtype=np.float32)
    rir = np.atleast_2d(np.asarray(rir, dtype=np.float32))
    S, (N, R) = spk.size, rir.shape
    K, P = -(-S // B), -(-R // B)
    xp = np.zeros((K + 1) * B, dtype=np.float32)
    xp[B:B + S] = spk
    X = scipy.fft.rfft(np.stack([xp[k * B:(k + 2) * B] for k in range(K)]), axis=-1)
    hp = np.zeros((N, P * B), dtype=np.float32)
    hp[:, :R] = rir
    H = scipy.fft.rfft(np.concatenate([hp.reshape(N, P, B), np.zeros((N, P, B), np.float32)], axis=-1), axis=-1)
    assert X.dtype == np.complex64 and H.dtype == np.complex64
    out = np.zeros((N, K * B), dtype=np.float32)
    for c in range(N):
        Y = np.zeros((K, B + 1), dtype=np.complex64)
        for p in range(P):
            Y[p:] += X[:K - p] * H[c, p]
        out[c] = scipy.fft.irfft(Y, n=2 * B, axis=-1)[:, B:].reshape(-1)
    return out[:, :S]


def add_room_response(spk, rir, conv=convolve64):
    revb = conv(spk, rir)
    return revb, np.mean(np.asarray(revb[0], dtype=np.float64)**2)


def _pick(rir, channel):
    rir = np.atleast_2d(rir)
    return rir[channel:channel + 1] if channel >= 0 else rir


def run_simu(case, conv=convolve64):
    """(mix, [speaker references], noise reference or None) as the reference's run_simu returns
    them (:244-312), every array float64."""
    ch, L = case["dump_channel"], mix_nsamps(case)
    spk_rir, noise_rir = case.get("spk_rir"), case.get("noise_rir")
    sdr = [0.0] + list(case.get("sdr", []))
    images, powers = [], []
    for i, s in enumerate(case["spk"]):
        s = pcm_to_float(s)
        if spk_rir is None:
            img = np.atleast_2d(s).astype(np.float64)
            p = np.mean(img[0]**2)
        else:
            img, p = add_room_response(s, _pick(pcm_to_float(spk_rir[i]), ch), conv)
        images.append(np.asarray(img, dtype=np.float64))
        powers.append(p)
    N = images[0].shape[0]
    spk = [np.zeros((N, L)) for _ in images]
    for i, img in enumerate(images):
        beg = case["spk_begin"][i]
        coeff = 1.0 if i == 0 else coeff_snr(powers[i], powers[0], sdr[i])
        spk[i][:, beg:beg + img.shape[-1]] += coeff * img
    spk_utt = sum(spk)
    mix = spk_utt.copy()
    spk_power = np.mean(spk_utt[0]**2)
    noise = None
    if case.get("noise"):
        imgs, pws, dur = [], [], 0
        for i, n in enumerate(case["noise"]):
            n = pcm_to_float(n)
            beg = case["noise_begin"][i]
            if not case.get("repeat"):
                dur = min(n.shape[-1], L - beg)
            else:
                dur = L - beg
                if n.shape[-1] < dur:
                    n = np.pad(n, (0, dur - n.shape[-1]), mode="wrap")
            if noise_rir is None:
                img = np.atleast_2d(n).astype(np.float64)
                p = np.mean(img[0, :dur]**2)
            else:
                img, p = add_room_response(n[:dur], _pick(pcm_to_float(noise_rir[i]), ch), conv)
            imgs.append(np.asarray(img, dtype=np.float64))
            pws.append(p)
        noise = np.zeros((imgs[0].shape[0], L))
        for i, img in enumerate(imgs):  # every noise over the LAST one's `dur` (:139-142)
            beg = case["noise_begin"][i]
            noise[:, beg:beg + dur] += coeff_snr(pws[i], spk_power, case["noise_snr"][i]) * img[:, :dur]
        if noise.shape[0] != N:
            raise RuntimeError("Channel mismatch")
        mix = spk_utt + noise
    iso_only = False
    if case.get("iso") is not None:
        iso = np.atleast_2d(pcm_to_float(case["iso"]))[:, case.get("iso_offset", 0):case.get("iso_offset", 0) + L]
        if N == 1 and iso.shape[0] > 1:
            if ch < 0:
                raise RuntimeError("Single channel mixture vs multi-channel isotropic noise")
            iso = iso[ch:ch + 1]
        elif N > 1 and iso.shape[0] != N:
            raise RuntimeError("Channel number mismatch")
        dur = min(L, iso.shape[-1])
        chunk = iso[0, :dur].astype(np.float64)
        coeff = coeff_snr(np.mean(chunk**2), spk_power, case["iso_snr"])
        mix[:, :dur] += coeff * chunk
        if noise is None:
            noise, iso_only = (coeff * chunk)[None], True
        else:
            noise[:, :dur] += coeff * chunk
    factor = case.get("norm_factor", 0.9) / (np.max(np.abs(mix)) + EPSILON)
    # (iso_only: the reference's `noise[0] * factor` is the first SAMPLE of its one-dimensional
    # noise there; the model keeps the whole chunk, callers take [0] where they mirror it)
    return mix * factor, [s[0] * factor for s in spk], None if noise is None else noise[0] * factor


def mix_nsamps(case):
    return max(b + np.asarray(s).size for b, s in zip(case["spk_begin"], case["spk"]))


def to_pcm16(x):
    """write_wav: astype(float32), then libsndfile's float -> PCM_16."""
    return np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * 32767.0).astype(np.int64).astype(np.int16)


def pcm_diff(a, b):
    """(worst difference in LSB, fraction of samples that differ) of two PCM_16 arrays."""
    d = np.abs(np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64))
    return int(d.max()), float(np.mean(d != 0))


# ---- the fixture cases: synthetic, a few thousand samples ----
def _speech(rng, n, amp=6000.0):
    """Band-limited noise under a slow envelope, as int16."""
    x = np.convolve(rng.standard_normal(n + 31), np.hanning(32) / 8.0, mode="valid")[:n]
    env = 0.3 + 0.7 * np.abs(np.sin(np.linspace(0.0, 3.0 + rng.random() * 3.0, n)))
    return np.rint(amp * x * env).astype(np.int16)


def _rir(rng, N, R, amp=12000.0):
    t = np.arange(R)
    h = rng.standard_normal((N, R)) * np.exp(-t / (R / 5.0)) * 0.15
    for c in range(N):
        h[c, 20 + 3 * c] = 1.0
    return np.rint(amp * h).astype(np.int16)


def make_case(name):
    """The inputs of a CASES entry (deterministic)."""
    kind, seed, opt = CASES[name]
    rng = np.random.default_rng(seed)
    N = 4
    c = dict(dump_channel=opt.get("dump_channel", -1), norm_factor=0.9)
    if kind == "far":  # two speakers at begins 700 / 0, SDR 3, a shorter noise at 300, an isotropic chunk
        c.update(spk=[_speech(rng, 3300), _speech(rng, 3700)], spk_begin=[700, 0], sdr=[3.0],
                 spk_rir=[_rir(rng, N, 600), _rir(rng, N, 520)],
                 noise=[_speech(rng, 1900, 3000.0)], noise_begin=[300], noise_snr=[5.0], noise_rir=[_rir(rng, N, 601)],
                 repeat=opt.get("repeat", False),
                 iso=np.stack([_speech(rng, 5000, 1500.0) for _ in range(N)]), iso_offset=500, iso_snr=8.0)
    elif kind == "close2":  # the close-talk forms: no RIRs
        c.update(spk=[_speech(rng, 3000), _speech(rng, 2500)], spk_begin=[0, 900], sdr=[-2.0],
                 noise=[_speech(rng, 5000, 3000.0)], noise_begin=[0], noise_snr=[10.0], repeat=False)
    elif kind == "close1":  # one speaker, nothing else
        c.update(spk=[_speech(rng, 2100)], spk_begin=[0])
    elif kind == "iso_only":
        c.update(spk=[_speech(rng, 2600)], spk_begin=[0], spk_rir=[_rir(rng, 2, 300)],
                 iso=np.stack([_speech(rng, 2600, 1500.0) for _ in range(2)]), iso_offset=0, iso_snr=12.0)
    return c


CASES = {
    # name: (kind, seed, options)
    "far": ("far", 11, {}),
    "far_repeat": ("far", 12, dict(repeat=True)),
    "far_ch1": ("far", 13, dict(dump_channel=1)),
    "far_ch1_repeat": ("far", 14, dict(dump_channel=1, repeat=True)),
    "close2": ("close2", 15, {}),
    "close1": ("close1", 16, {}),
    "iso_only": ("iso_only", 17, {}),
}
# the cases that also go through the command lines (with the doc-derived case)
CLI_CASES = ("far",)


def cli_args(case, paths, mix, ref_dir=""):
    """The argument list of wav_simulate.py for a case whose arrays lie in the files `paths`
    (dict: spk, spk_rir, noise, noise_rir lists, iso)."""
    a = [mix, "--src-spk", ",".join(paths["spk"])]
    if paths.get("spk_rir"):
        a += ["--src-rir", ",".join(paths["spk_rir"])]
    if len(case["spk"]) > 1:
        a += ["--src-sdr=" + ",".join(str(v) for v in case["sdr"])]
    a += ["--src-begin=" + ",".join(str(v) for v in case["spk_begin"])]
    if case.get("noise"):
        a += ["--point-noise", ",".join(paths["noise"]), "--point-noise-snr=" + ",".join(str(v) for v in case["noise_snr"]),
              "--point-noise-begin=" + ",".join(str(v) for v in case["noise_begin"]),
              "--point-noise-repeat", "true" if case.get("repeat") else "false"]
        if paths.get("noise_rir"):
            a += ["--point-noise-rir", ",".join(paths["noise_rir"])]
    if case.get("iso") is not None:
        a += ["--isotropic-noise", paths["iso"], "--isotropic-noise-snr=" + str(case["iso_snr"]),
              "--isotropic-noise-offset", str(case.get("iso_offset", 0))]
    a += ["--dump-channel", str(case["dump_channel"]), "--norm-factor", str(case["norm_factor"])]
    if ref_dir:
        a += ["--dump-ref-dir", ref_dir]
    return a


def write_case_files(case, tmp):
    """The arrays of a case as 16 kHz PCM_16 files under tmp; returns the `paths` of cli_args."""
    import os
    import scipy.io.wavfile as wavfile
    paths = {}
    for key in ("spk", "spk_rir", "noise", "noise_rir"):
        if case.get(key):
            paths[key] = []
            for i, a in enumerate(case[key]):
                p = os.path.join(tmp, f"{key}{i}.wav")
                a = np.asarray(a, dtype=np.int16)
                wavfile.write(p, 16000, a.T if a.ndim == 2 else a)
                paths[key].append(p)
    if case.get("iso") is not None:
        paths["iso"] = os.path.join(tmp, "iso.wav")
        a = np.asarray(case["iso"], dtype=np.int16)
        wavfile.write(paths["iso"], 16000, a.T if a.ndim == 2 else a)
    return paths


def fftconvolve64(spk, rir):
    """convolve64 through a float64 FFT (error about 1e-16 of the peak): for the long cases."""
    import scipy.signal
    spk = np.asarray(spk, dtype=np.float64)
    return np.stack([scipy.signal.fftconvolve(spk, h)[:spk.size] for h in np.atleast_2d(np.asarray(rir, np.float64))])


# ---- the fixtures (tools/make_simu_golden.py) ----
def _golden(name):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))


def load_case(gold, name):
    """(case, reference) of a CASES entry out of ref_simu.npz: the inputs as make_case built them
    and the reference's (mix, [spk], noise or None), e_ref and, for CLI_CASES, its PCM_16 files."""
    case = make_case(name)
    for key in ("spk", "spk_rir", "noise", "noise_rir"):
        if case.get(key):
            case[key] = [gold[f"{name}_in_{key}_{i}"] for i in range(len(case[key]))]
    if case.get("iso") is not None:
        case["iso"] = gold[f"{name}_in_iso"]
    ref = dict(mix=gold[f"{name}_mix"], spk=[gold[f"{name}_spk{i}"] for i in range(len(case["spk"]))],
               noise=gold[f"{name}_noise"] if f"{name}_noise" in gold.files else None,
               e_ref=float(gold[f"{name}_e_ref"]))
    ref["cli"] = {k[len(name) + 5:]: gold[k] for k in gold.files if k.startswith(name + "_cli_")}
    return case, ref


def load_doc_case():
    """The doc-derived case: (case, the reference's PCM_16 files, e_ref)."""
    gi, go = _golden("ref_simu_doc_in.npz"), _golden("ref_simu_doc_out.npz")
    case = dict(spk=[gi["spk_0"], gi["spk_1"]], spk_begin=[16000, 0], sdr=[3.0], spk_rir=[gi["spk_rir_0"], gi["spk_rir_1"]],
                noise=[gi["noise_0"]], noise_begin=[0], noise_snr=[5.0], noise_rir=[gi["noise_rir_0"]], repeat=False,
                iso=np.stack([gi["iso0"]] * 4), iso_offset=0, iso_snr=8.0, dump_channel=-1, norm_factor=0.9)
    return case, {k[4:]: go[k] for k in go.files if k.startswith("cli_")}, float(go["e_ref"])


def worst_error(got, ref):
    """Worst |got - ref| over the reference's peak, over mix, speaker references and noise
    reference; got as (mix, [spk], noise) in any float type, compared as float32 (the fixture
    stores the reference's float64 arrays rounded to float32)."""
    peak = float(np.max(np.abs(ref["mix"])))
    pairs = [(np.squeeze(got[0]), ref["mix"])] + list(zip(got[1], ref["spk"]))
    if ref["noise"] is not None:
        pairs.append((got[2], ref["noise"]))
    return max(float(np.max(np.abs(np.asarray(a, dtype=np.float32).astype(np.float64) - np.asarray(b, np.float64))))
               for a, b in pairs) / peak
