"""
float64 numpy restatement of mask-based sound source localisation as funcwj/setk runs it
(scripts/sptk/libs/ssl.py:12-110, do_ssl.py:80-114).  Written from the formulas, none of the
reference's text; tests/test_ssl_model.py checks it against recorded indices of the unmodified
reference (tests/golden/ref_ssl.npz).  Every function returns the score spectrum as well as the
index, so that the GPU tests can bound the spectrum and apply the gap rule to the index.

    ML     sv <- sv / ||sv||_2 (microphones); x <- x / max(|x|, eps) when norm
           delta[a,t,f] = sum_m |x|^2 - |sum_m sv conj(x)|^2 / (1 + eps)
           ll = -log(max(delta, eps)) (compression <= 0) | -delta^compression
           score[a] = sum_{t,f} mask ll;  argmax
    SRP    score[a] = sum_{t,f} mask mean_p cos((arg x_l - arg x_r) - (arg sv_l - arg sv_r));  argmax
    MUSIC  R_f = (x mask)(x mask)^H / T, E_n = all eigenvectors but the principal one,
           score[a] = sum_f |sv^H E_n E_n^H sv|;  argmin
SRP and MUSIC are kept in the reference's own form (angles and cosines; the full noise
subspace out of eigh): the device's factorised SRP and its principal-eigenvector MUSIC are
reformulations that the tests check against this, not assume.
"""
import numpy as np

EPSILON = np.finfo(np.float32).eps  # libs/utils.py:16, what do_ssl.py passes to ml_ssl


def ml_ssl(stft, sv, compression=0, eps=1e-8, norm=False, mask=None):
    """stft M x T x F, sv A x M x F, mask T x F | N x T x F | None -> (index, score [A] | [N][A])."""
    x = np.asarray(stft).astype(np.complex128)
    sv = np.asarray(sv).astype(np.complex128)
    _, T, F = x.shape
    mask = np.ones((T, F)) if mask is None else np.asarray(mask, dtype=np.float64)
    sv = sv / np.sqrt(np.sum(np.abs(sv)**2, axis=1, keepdims=True))
    if norm:
        x = x / np.maximum(np.abs(x), eps)
    power = np.sum(np.abs(x)**2, axis=0)                              # T x F
    proj = np.abs(np.einsum("amf,mtf->atf", sv, x.conj()))**2         # A x T x F
    delta = power[None] - proj / (1 + eps)
    with np.errstate(invalid="ignore"):
        ll = -np.log(np.maximum(delta, eps)) if compression <= 0 else -np.power(delta, compression)
    score = np.einsum("...tf,atf->...a", mask, ll)
    return np.argmax(score, axis=-1), score


def srp_ssl(stft, sv, srp_pair, mask=None):
    x, sv = np.asarray(stft).astype(np.complex128), np.asarray(sv).astype(np.complex128)
    _, T, F = x.shape
    mask = np.ones((T, F)) if mask is None else np.asarray(mask, dtype=np.float64)
    left, right = [list(p) for p in srp_pair]
    obs, ora = np.angle(x), np.angle(sv)
    obs_ipd = obs[left] - obs[right]                                  # P x T x F
    ora_ipd = ora[:, left] - ora[:, right]                            # A x P x F
    score = np.zeros(sv.shape[0])
    for a in range(sv.shape[0]):                                      # (A x P x T x F at once is large)
        score[a] = np.sum(np.mean(np.cos(obs_ipd - ora_ipd[a][:, None, :]), axis=0) * mask)
    return int(np.argmax(score)), score


def music_ssl(stft, sv, mask=None):
    x, sv = np.asarray(stft).astype(np.complex128), np.asarray(sv).astype(np.complex128)
    _, T, F = x.shape
    mask = np.ones((T, F)) if mask is None else np.asarray(mask, dtype=np.float64)
    obs = (x * mask[None]).transpose(2, 0, 1)                         # F x M x T
    R = np.matmul(obs, obs.conj().transpose(0, 2, 1)) / T
    _, v = np.linalg.eigh(R)                                          # ascending
    En = v[..., :-1]                                                  # F x M x (M - 1)
    proj = np.matmul(En, En.conj().transpose(0, 2, 1))                # F x M x M
    s = sv.transpose(2, 0, 1)                                         # F x A x M
    score = np.sum(np.abs(np.einsum("fam,fmn,fan->fa", s.conj(), proj, s)), axis=0)
    return int(np.argmin(score)), score


def get_doa(backend, stft, sv, mask=None, srp_pair=None):
    """get_doa of do_ssl.py:30-37 -> (index, score)."""
    if srp_pair:
        return srp_ssl(stft, sv, srp_pair, mask=mask)
    if backend == "ml":
        return ml_ssl(stft, sv, mask=mask, compression=-1, eps=EPSILON)
    return music_ssl(stft, sv, mask=mask)


def online_windows(num_frames, chunk_len, look_back):
    """do_ssl.py:103-104: [max(t - look_back, 0), t + chunk_len) for t = 0, chunk_len, ...
    (clipped to the utterance, as a numpy slice clips)."""
    return [(max(t - look_back, 0), min(t + chunk_len, num_frames)) for t in range(0, num_frames, chunk_len)]


def windowed(backend, stft, sv, windows, mask=None, srp_pair=None):
    """One get_doa per window of FRAMES, mask sliced along the frames as well (the evident intent
    of do_ssl.py:105-111; see tests/PARITY_NOTES_SSL.md) -> (indices [W], scores [W][A])."""
    idx, sc = [], []
    for t0, t1 in windows:
        i, s = get_doa(backend, stft[:, t0:t1], sv, None if mask is None else mask[t0:t1], srp_pair)
        idx.append(int(i))
        sc.append(s)
    return np.array(idx), np.stack(sc)


def gap(score, take_min=False):
    """Distance between the best and the runner-up score, relative to the spread of the spectrum."""
    s = np.sort(np.asarray(score, dtype=np.float64))
    spread = s[-1] - s[0]
    return float((s[1] - s[0]) if take_min else (s[-1] - s[-2])) / spread


def steer_vectors(geometry, num_doas, num_bins, topo=None, around=6, radius=0.05, center=False, c=343.0,
                  sr=16000):
    """compute_steer_vector.py:17-51 -> A x M x F."""
    from setk_amd.libs.beamformer import circular_steer_vector, linear_steer_vector
    if geometry == "linear":
        sv = [linear_steer_vector(np.array(topo), d, num_bins, c=c, sr=sr) for d in np.linspace(0, 180, num_doas)]
    else:
        sv = [circular_steer_vector(radius, around, d, num_bins, c=c, sr=sr, center=center)
              for d in np.arange(0, 360, 360 / num_doas)]
    return np.stack(sv).transpose(0, 2, 1)


def synth_scene(seed, geometry, C, doa, frames, snr_db, hop=256, c=343.0, sr=16000):
    """A plane wave from `doa` degrees on a linear (5 cm spacing) or circular (5 cm radius) array
    of C microphones plus independent sensor noise: the source is amplitude-modulated coloured
    noise, delayed per microphone in the frequency domain by the steer vector of the whole
    signal's transform.  Returns float32 C x N with N = hop (frames - 1), |x| <= 0.5."""
    from setk_amd.libs.beamformer import circular_steer_vector, linear_steer_vector
    rng = np.random.default_rng(seed)
    N = hop * (frames - 1)
    env = np.repeat(rng.uniform(0.1, 1.0, size=N // 800 + 1), 800)[:N]
    src = np.convolve(rng.laplace(size=N) * env, 0.6**np.arange(32))[:N]
    nb = N // 2 + 1
    if geometry == "linear":
        d = linear_steer_vector(np.arange(C) * 0.05, doa, nb, c=c, sr=sr)
    else:
        d = circular_steer_vector(0.05, C, doa, nb, c=c, sr=sr)
    mix = np.fft.irfft(np.fft.rfft(src)[:, None] * d, n=N, axis=0).T          # C x N
    noise = rng.normal(size=mix.shape)
    noise *= np.sqrt(np.mean(mix**2) / np.mean(noise**2)) * 10**(-snr_db / 20)
    mix = mix + noise
    mix *= 0.5 / np.max(np.abs(mix))
    return mix.astype(np.float32)


# ---- the synthetic scenes of tests/golden/ref_ssl.npz (tools/make_ssl_golden.py) ----
# name -> seed, geometry, channels, DoA (degrees), frames, SNR (dB), directions, frame length (hop = half)
SCENES = {
    "c2": (31, "linear", 2, 60.0, 30, 15.0, 37, 512),
    "c4": (32, "linear", 4, 110.0, 30, 10.0, 37, 512),
    "c8": (33, "circular", 8, 200.0, 30, 10.0, 37, 512),
    "odd": (34, "linear", 3, 45.0, 37, 15.0, 5, 256),
}


def scene_stft_kwargs(name):
    n = SCENES[name][7]
    return dict(frame_len=n, frame_hop=n // 2, window="hann", center=True, round_power_of_two=True)


def scene_samples(name):
    seed, geometry, C, doa, frames, snr, _, n = SCENES[name]
    return synth_scene(seed, geometry, C, doa, frames, snr, hop=n // 2)


def scene_steer_vectors(name):
    """The candidate directions of a scene: 0 .. 180 degrees for the linear arrays (5 cm spacing),
    the full circle for the circular one (5 cm radius)."""
    _, geometry, C, _, _, _, A, n = SCENES[name]
    return steer_vectors(geometry, A, n // 2 + 1, topo=np.arange(C) * 0.05, around=C, radius=0.05)


def scene_pairs(name):
    """SRP pairs: neighbours on a line, opposite microphones on the circle."""
    _, geometry, C = SCENES[name][:3]
    if geometry == "circular":
        return list(range(C // 2)), [i + C // 2 for i in range(C // 2)]
    return list(range(C - 1)), list(range(1, C))


def scene_masks(name, count=2):
    """`count` deterministic T x F masks in (0, 1) (float32), smooth along both axes."""
    seed, _, _, _, frames, _, _, n = SCENES[name]
    rng = np.random.default_rng(1000 + seed)
    F = n // 2 + 1
    out = []
    for _ in range(count):
        m = rng.uniform(size=(frames + 4, F + 4))
        m = sum(m[i:i + frames, j:j + F] for i in range(5) for j in range(5)) / 25.0
        out.append(np.clip(2.0 * m - 0.5, 0.02, 1.0).astype(np.float32))
    return out
