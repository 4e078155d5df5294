"""
The float64 model of the image-method RIR generator (the reference's include/rir-generator.cc:108-223
restated in numpy) and the cases of tests/golden/ref_rir.npz.

The inputs are the reference's float32 values (BaseFloat after parsing); from there geometry,
fractional delay and sums are float64, which is what the device kernel (setk_amd/csrc/rir.hip)
computes as well.  The reference itself works in float32 (`dist` is a float, the taps are summed in
float): its distance to this model is each case's `e_ref` in the fixture.
"""
import numpy as np

MIC_TYPES = {"bidirectional": 0, "hypercardioid": 1, "cardioid": 2, "subcardioid": 3, "omnidirectional": 4}
RHO = {0: 0.0, 1: 0.25, 2: 0.5, 3: 0.75, 4: 1.0}


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def case(room, src, mics, beta=None, rt60=None, num_samples=512, fs=16000.0, c=340.0, order=-1, hp=True,
         mic_type="omnidirectional", angle=(0.0, 0.0)):
    """One case: either six coefficients (`beta`) or a reverberation time (`rt60`)."""
    return dict(room=_f32(room), src=_f32(src), mics=_f32(mics).reshape(-1, 3),
                beta=None if beta is None else _f32(beta), rt60=None if rt60 is None else float(np.float32(rt60)),
                num_samples=int(num_samples), fs=float(np.float32(fs)), c=float(np.float32(c)), order=int(order),
                hp=bool(hp), mic_type=mic_type, angle=_f32(angle))


def cases():
    """The fixture's cases: the smallest shapes at which the kernel can still go wrong."""
    room, src, mic = (4.0, 5.0, 2.5), (1.2, 1.7, 1.4), (2.6, 3.1, 1.1)
    line16 = [(1.0 + 0.11 * i, 2.0 + 0.03 * i, 1.2 + 0.01 * i) for i in range(16)]
    out = {
        "small": case(room, src, [mic], rt60=0.3),
        # 5 cm: pos = fdist - Tw / 2 + 1 is negative, the window is clipped at tap 0
        "near": case(room, (2.6, 3.15, 1.1), [mic], rt60=0.3, num_samples=384),
        # cts = 250 / 16000 = 2^-6 and 0.5 m on one axis: dist = 32 exactly, d = 0
        "integer_delay": case(room, (1.0, 1.5, 1.25), [(1.5, 1.5, 1.25)], rt60=0.45, c=250.0, num_samples=384),
        "six_betas": case(room, src, [mic], beta=(0.9, 0.8, 0.7, 0.6, 0.5, 0.85), num_samples=400),
        "order2": case(room, src, [mic], rt60=0.3, order=2, num_samples=640),
        "no_hp": case(room, src, [mic], rt60=0.3, hp=False, num_samples=333),
        "anechoic": case(room, src, [mic], rt60=0.0, num_samples=256),
        "array16": case((5.0, 4.0, 3.0), (3.9, 1.1, 1.7), line16, rt60=0.35, num_samples=300),
        # one tap: only an image closer than one sample (2 cm) reaches it
        "taps_1": case(room, (2.6, 3.11, 1.1), [mic], rt60=0.3, num_samples=1),
        "workload": case((7.0, 8.0, 3.0), (2.1, 5.3, 1.6), [(3.4, 0.7, 1.3), (3.5, 0.7, 1.3)], rt60=0.4,
                         num_samples=8000),
    }
    for name in ("bidirectional", "hypercardioid", "cardioid", "subcardioid"):
        out["pattern_" + name] = case(room, src, [mic, (2.0, 1.0, 1.9)], rt60=0.3, mic_type=name, angle=(0.6, 0.3),
                                      num_samples=300)
    return out


def beta_of(c):
    """The six float32 coefficients of a case: its own, or rir-generator.cc:78-92 on its rt60 in the
    reference's float32 steps (setk_amd.libs.rir.beta_from_rt60 is the product's copy; this one keeps
    the tests independent of it)."""
    if c["beta"] is not None:
        return c["beta"]
    if c["rt60"] == 0:
        return np.zeros(6, np.float32)
    x, y, z = c["room"]
    V, S = x * y * z, np.float32(2) * (x * y + x * z + y * z)
    alfa = np.float32(np.float64(np.float32(24) * V) * np.log(10.0) /
                      np.float64(np.float32(c["c"]) * S * np.float32(c["rt60"])))
    if alfa > 1:
        raise RuntimeError(f"{alfa} > 1: The reflection coefficients cannot be calculated")
    return np.full(6, np.sqrt(np.float32(1) - alfa), np.float32)


def generate(c, beta=None, boundary=None):
    """[n_mics][num_samples] float64.  boundary: a list that receives min |dist - num_samples| over
    the images that pass the order test (the condition on the fixture's inputs)."""
    from scipy.signal import lfilter
    beta = np.asarray(beta_of(c) if beta is None else beta, np.float64)
    fs, vel, ns, order = np.float64(c["fs"]), np.float64(c["c"]), c["num_samples"], c["order"]
    cts = vel / fs
    S, T = np.float64(c["src"]) / cts, np.float64(c["room"]) / cts
    Tw = 2 * int(0.004 * fs + 0.5)
    rho = RHO[MIC_TYPES[c["mic_type"]]]
    a0, a1 = np.float64(c["angle"])
    n = np.arange(Tw)
    nn = [int(np.ceil(ns / (2 * T[a]))) for a in range(3)]
    # per axis: every (cell, mirror) pair, mirror fastest, as the reference nests them
    axes = []
    for a in range(3):
        cell = np.repeat(np.arange(-nn[a], nn[a] + 1), 2)
        mirror = np.tile(np.arange(2), 2 * nn[a] + 1)
        refl = beta[2 * a] ** np.abs(cell - mirror) * beta[2 * a + 1] ** np.abs(cell)
        axes.append((cell, mirror, refl))
    out = np.zeros((len(c["mics"]), ns))
    for m, mic in enumerate(np.float64(c["mics"]) / cts):
        comp = [(1 - 2 * mi) * S[a] - mic[a] + 2 * ce * T[a] for a, (ce, mi, _) in enumerate(axes)]
        hops = [np.abs(2 * ce - mi) for ce, mi, _ in axes]
        acc = np.zeros(ns)
        # x slabs keep the working set small (the workload case has 1.3 M candidates per channel)
        for ix in range(len(comp[0])):
            px, py, pz = comp[0][ix], comp[1][:, None], comp[2][None, :]
            dist = np.sqrt(px * px + py * py + pz * pz)
            ok = np.ones_like(dist, bool) if order == -1 else (hops[0][ix] + hops[1][:, None] + hops[2][None, :] <= order)
            if boundary is not None and ok.any():
                boundary.append(np.min(np.abs(dist[ok] - ns)))
            fd = np.floor(dist)
            ok &= fd < ns
            if not ok.any():
                continue
            iy, iz = np.nonzero(ok)
            dist, fd = dist[ok], fd[ok]
            refl = axes[0][2][ix] * axes[1][2][iy] * axes[2][2][iz]
            if rho == 1.0:
                pat = 1.0
            else:
                qx, qy, qz = np.full(dist.shape, px), comp[1][iy], comp[2][iz]
                theta, phi = np.arccos(qz / dist), np.arctan2(qy, qx)
                pat = rho + (1 - rho) * (np.sin(np.pi / 2 - a1) * np.sin(theta) * np.cos(a0 - phi) +
                                         np.cos(np.pi / 2 - a1) * np.cos(theta))
            gain = pat * refl / (4 * np.pi * dist * cts)
            frac = (dist - fd)[:, None]
            t = n[None, :] + 1 - frac
            x = np.pi * (t - Tw // 2)
            with np.errstate(invalid="ignore", divide="ignore"):
                sinc = np.where(x == 0, 1.0, np.sin(x) / x)
            val = gain[:, None] * (0.5 * (1 - np.cos(2 * np.pi * (t / Tw))) * sinc)
            tap = (fd.astype(np.int64) - Tw // 2 + 1)[:, None] + n[None, :]
            keep = (tap >= 0) & (tap < ns)
            acc += np.bincount(tap[keep], weights=val[keep], minlength=ns)
        if c["hp"]:
            W = 2 * np.pi * 100 / fs
            R1 = np.exp(-W)
            acc = lfilter([1.0, -1 - R1, R1], [1.0, -2 * R1 * np.cos(W), R1 * R1], acc)
        out[m] = acc
    return out


def load_fixture(path=None):
    """tests/golden/ref_rir.npz as {name: (case, the reference's RIR, e_ref, its seconds per channel)};
    a case carries the six coefficients the generator used (`beta`) and, where it was given one,
    the reverberation time (`rt60`)."""
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_rir.npz")
    z = np.load(path)
    names = {v: k for k, v in MIC_TYPES.items()}
    out = {}
    for name in sorted({k.split("/")[0] for k in z.files} - {"cli"}):
        g = lambda k: z[f"{name}/{k}"]  # noqa: E731
        ns, order, hp, mic = (int(v) for v in g("ints"))
        c = dict(room=g("room"), src=g("src"), mics=g("mics"), beta=g("beta"), angle=g("angle"),
                 rt60=None if float(g("rt60")) < 0 else float(g("rt60")), num_samples=ns, order=order, hp=bool(hp),
                 mic_type=names[mic], fs=float(g("fs_c")[0]), c=float(g("fs_c")[1]))
        out[name] = (c, g("rir"), float(g("e_ref")), float(g("sec_per_channel")))
    return out


def load_cli_fixture(name, path=None):
    """What the reference's `name`.py (rir_generate_1d / rir_generate_2d) did with `random` seeded:
    (its arguments, the seed, the text of its rir.json, the generator's float32 matrix of
    Room1-1.wav before rir-simulate.cc:64's scaling)."""
    import json
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_rir.npz")
    z = np.load(path)
    g = lambda k: z[f"cli/{name}/{k}"]  # noqa: E731
    return json.loads(g("args").tobytes().decode()), int(g("seed")), g("rir_json").tobytes().decode(), g("room1_1")
