"""
Oracle TF masks, mask-based separation and oracle separation on the device, every form judged per
cell (masks) or per block of hop samples (waves) by tests/tfmask_cases.py; figures and bars in
tests/PARITY_NOTES_TFMASK.md.  The float64 references are computed once per module and shared.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import stft_cases as sc
import tfmask_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 257
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def pairs(which):
    return cached(("pairs", which), getattr(tc, which))


def new_ctx(geo):
    from setk_amd import _ffi
    c = _ffi.Context(0)
    c.stft_plan(*geo.plan_args())
    return c


@pytest.fixture(scope="module")
def ctxs():
    """One handle per geometry of the cases (centred, uncentred)."""
    made = {}

    def get(geo):
        key = repr(geo)
        if key not in made:
            made[key] = new_ctx(geo)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def dev():
    import torch
    return torch.device("cuda:0")


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def width(kind):
    return 2 * F if kind == "crm" else F


def mask_batch(c, kind, group, cutoff, pcm=False):
    """setk_tf_mask_batch on a list of pairs: (masks, statistics, status)."""
    import torch
    from setk_amd import _ffi
    if pcm:
        t = [to_dev(p.pcm[0][0]) for p in group]
        m = [to_dev(p.pcm[1]) for p in group]
    else:
        t = [to_dev(p.tgt) for p in group]
        m = [to_dev(p.mix) for p in group]
    ns = [p.mix.shape[0] for p in group]
    out = [torch.full((c.num_frames(n), width(kind)), float("nan"), dtype=torch.float32, device=dev()) for n in ns]
    status = np.full(len(group), -1, np.int32)
    stats = c.tf_mask_batch(kind, [x.data_ptr() for x in t], [x.data_ptr() for x in m], ns,
                            [x.data_ptr() for x in out], cutoff=cutoff, status=status,
                            flags=_ffi.FLAG_IN_PCM16 if pcm else 0)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], stats, status


def check_stats(raw, got, stats, cutoff, name):
    """The device's clipped mask and its three numbers against numpy on the device's own unclipped
    mask: bit for bit, the counts exactly, the sum to 1e-12 relative."""
    want, (over, below, below_sum) = tc.clip_formula(raw, cutoff)
    assert np.array_equal(want, got, equal_nan=True), f"{name}: the clips differ from numpy's on the same mask"
    assert stats[0] == over and stats[1] == below, f"{name}: counts {stats[:2]} against {(over, below)}"
    assert abs(stats[2] - below_sum) <= 1e-12 * abs(below_sum), f"{name}: sum {stats[2]!r} against {below_sum!r}"


def by_geometry(group):
    out = {}
    for p in group:
        out.setdefault(repr(p.geo), []).append(p)
    return list(out.values())


# ---------------------------------------------------------------- 1. masks
@pytest.mark.parametrize("kind", tc.KINDS)
def test_masks_on_stored_spectra(ctxs, kind):
    """setk_tf_mask on the float64 spectra rounded to complex64 (device memory), cutoff -1 and 2."""
    fails, lines = [], []
    for p in pairs("noise_pairs"):
        c = ctxs(p.geo)
        ts, m = p.spectra(np.complex64)
        d_t, d_m = to_dev(ts[0]), to_dev(m)
        import torch
        raw = torch.full((p.T, width(kind)), float("nan"), dtype=torch.float32, device=dev())
        c.tf_mask(kind, d_t, d_m, p.T, F, raw, cutoff=float("nan"), want_stats=False)
        raw = raw.cpu().numpy()
        for cutoff in tc.CUTOFFS:
            out = torch.full((p.T, width(kind)), float("nan"), dtype=torch.float32, device=dev())
            stats = c.tf_mask(kind, d_t, d_m, p.T, F, out, cutoff=cutoff)
            got = out.cpu().numpy()
            check_stats(raw, got, stats, cutoff, f"{p.name}:{kind}@{cutoff}")
            v = tc.judge_mask(f"{p.name}:{kind}@{cutoff} (stored spectra)", kind, got, p, cutoff)
            lines.append(v.line())
            fails += v.failures
    print("\n".join(lines))
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("pcm", [False, True])
@pytest.mark.parametrize("kind", tc.KINDS)
def test_masks_fused_batch(ctxs, kind, pcm):
    """setk_tf_mask_batch, float32 and int16 input, cutoff -1 and 2."""
    fails, lines = [], []
    for group in by_geometry(pairs("noise_pairs")):
        c = ctxs(group[0].geo)
        raws, _, _ = mask_batch(c, kind, group, float("nan"), pcm)
        for cutoff in tc.CUTOFFS:
            outs, stats, status = mask_batch(c, kind, group, cutoff, pcm)
            for p, raw, got, st, code in zip(group, raws, outs, stats, status):
                name = f"{p.name}:{kind}@{cutoff} (fused, {'int16' if pcm else 'float32'})"
                check_stats(raw, got, st, cutoff, name)
                assert code == (3 if not np.isfinite(got).all() else 0), name
                v = tc.judge_mask(name, kind, got, p, cutoff)
                lines.append(v.line())
                fails += v.failures
    print("\n".join(lines))
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------- 2. special cells
@pytest.mark.parametrize("kind", tc.KINDS)
def test_special_cells(ctxs, kind):
    """zeros (silence in the target only, the mixture only, both), the 16-bit extremes and the
    quiet pair: NaN / +-inf / exact zeros on exactly the reference's cells (judge_mask), with and
    without cutoff; status is SETK_NUM_NONFINITE exactly where a NaN / inf is delivered; int16
    input gives the bits of its float32 twin."""
    fails, lines = [], []
    group = pairs("zeros_pairs") + pairs("pcm_pairs") + pairs("quiet_pairs")
    c = ctxs(group[0].geo)
    seen_special = 0
    for cutoff in tc.CUTOFFS:
        outs, _, status = mask_batch(c, kind, group, cutoff)
        twins = [p for p in group if p.pcm is not None]
        outs16, _, status16 = mask_batch(c, kind, twins, cutoff, pcm=True)
        by_name = {p.name: (o, s) for p, o, s in zip(twins, outs16, status16)}
        for p, got, code in zip(group, outs, status):
            name = f"{p.name}:{kind}@{cutoff}"
            special = int((~np.isfinite(got)).sum())
            seen_special += special
            assert code == (3 if special else 0), f"{name}: status {code} with {special} NaN / inf cells"
            if p.name in by_name:
                assert np.array_equal(by_name[p.name][0], got, equal_nan=True), f"{name}: int16 and float32 differ"
                assert by_name[p.name][1] == code
            if p.judged:
                v = tc.judge_mask(name, kind, got, p, cutoff)
                lines.append(v.line())
                fails += v.failures
    print("\n".join(lines))
    if kind in ("iam", "psm"):
        assert seen_special > 0     # (0 / 0 in the frames silent on both sides)
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------- 3. separation with a given mask
def given_mask(p, seed):
    rng = np.random.default_rng(seed)
    return (1.5 * rng.random((p.T, F)) ** 2).astype(np.float32)


def separate(c, group, masks, refs=None, norm=None, nsamps=None, pcm=False, out16=False):
    import torch
    from setk_amd import _ffi
    m = [to_dev(p.pcm[1] if pcm else p.mix) for p in group]
    # refs[i] true: the pair's own target is the phase reference (in the input's format)
    r = None if refs is None else [to_dev(p.pcm[0][0] if pcm else p.tgt) if use else None
                                   for p, use in zip(group, refs)]
    k = [to_dev(x) for x in masks]
    ns = [p.mix.shape[0] for p in group]
    L = [c.istft_num_samples(c.num_frames(n), None if nsamps is None or nsamps[i] < 0 else nsamps[i])
         for i, n in enumerate(ns)]
    out = [torch.full((n,), 32000 if out16 else float("nan"), dtype=torch.int16 if out16 else torch.float32,
                      device=dev()) for n in L]
    status = np.full(len(group), -1, np.int32)
    c.tf_separate_batch([x.data_ptr() for x in m], ns, [x.data_ptr() for x in k], [x.data_ptr() for x in out],
                        phase_ptrs=None if r is None else [None if x is None else x.data_ptr() for x in r],
                        norm=norm, nsamps=nsamps, status=status,
                        flags=(_ffi.FLAG_IN_PCM16 if pcm else 0) | (_ffi.FLAG_OUT_PCM16 if out16 else 0))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], status


@pytest.mark.parametrize("form", ["mask", "phase-ref", "keep-length", "mixed-norm"])
def test_separation_with_a_given_mask(ctxs, form):
    fails, lines = [], []
    for group in by_geometry(pairs("noise_pairs")[1:]):
        c = ctxs(group[0].geo)
        masks = [given_mask(p, 7 + i) for i, p in enumerate(group)]
        refs = [True] * len(group) if form == "phase-ref" else None
        nsamps = [p.mix.shape[0] for p in group] if form == "keep-length" else None
        # mixed norm on for every other utterance, off (<= 0) for the rest
        norm = [float(np.abs(p.mix).max()) if i % 2 == 0 else -1.0 for i, p in enumerate(group)] \
            if form == "mixed-norm" else None
        outs, status = separate(c, group, masks, refs, norm, nsamps)
        for i, (p, mk, got) in enumerate(zip(group, masks, outs)):
            assert status[i] == 0
            y, y32, inp = tc.wave_reference(p, [mk], phase_ref=None if refs is None else p.tgt,
                                            nsamps=None if nsamps is None else nsamps[i],
                                            norm=None if norm is None else norm[i])[0]
            v = tc.judge_wave(f"{p.name} separation ({form})", got, y, y32, inp, p.geo.hop)
            lines.append(v.line())
            fails += v.failures
    print("\n".join(lines))
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------- 4. oracle separation
def oracle(c, kind, group, nsamps=None, pcm=False):
    import torch
    from setk_amd import _ffi
    K = len(group[0].targets)
    m = [to_dev(p.pcm[1] if pcm else p.mix) for p in group]
    t = [to_dev(p.pcm[0][k] if pcm else p.targets[k]) for p in group for k in range(K)]
    ns = [p.mix.shape[0] for p in group]
    out = [torch.full((c.istft_num_samples(c.num_frames(n), None if nsamps is None else nsamps[i]),), float("nan"),
                      dtype=torch.float32, device=dev()) for i, n in enumerate(ns) for _ in range(K)]
    status = np.full(len(group), -1, np.int32)
    c.oracle_separate_batch(kind, K, [x.data_ptr() for x in m], [x.data_ptr() for x in t], ns,
                            [x.data_ptr() for x in out], nsamps=nsamps, status=status,
                            flags=_ffi.FLAG_IN_PCM16 if pcm else 0)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], status


@pytest.mark.parametrize("kind", tc.ORACLE_KINDS)
def test_oracle_separation(ctxs, kind):
    """K = 2, 3, 8; for irm and ibm the K waves sum to the inverse of the mixture's own spectrum
    (the masks sum to one) within the summed allowance."""
    fails, lines = [], []
    for p in pairs("oracle_pairs"):
        assert tc.ibm_band_cells(p) == 0
        c = ctxs(p.geo)
        K = len(p.targets)
        outs, status = oracle(c, kind, [p])
        assert status[0] == 0
        ts, m = p.spectra()
        masks = [np.asarray(x, np.float64) for x in tc.oracle_formula(kind, m, ts)]
        extra = [tc.oracle_wave_extra(kind, p, k, masks[k]) for k in range(K)]
        refs = tc.wave_reference(p, masks, a_mask=extra)
        for k in range(K):
            y, y32, inp = refs[k]
            v = tc.judge_wave(f"{p.name} oracle {kind} speaker {k + 1}", outs[k], y, y32, inp, p.geo.hop)
            lines.append(v.line())
            fails += v.failures
        if kind in ("irm", "ibm"):
            # the summed allowance: every speaker's own (its yardstick term and its input-referred
            # term) added up per block; judge() then takes the reference as its own yardstick
            hop = p.geo.hop
            ysum = sum(r[0] for r in refs)
            each = [sc.M_BITS * np.maximum(np.linalg.norm(sc.blocks(y32 - y, hop), axis=1),
                                           sc.U32 * np.linalg.norm(sc.blocks(y, hop), axis=1)) + inp
                    for y, y32, inp in refs]
            whole = sc.ref_istft(m, p.geo)
            if kind == "ibm":
                assert np.abs(ysum - whole).max() <= 1e-12 * np.abs(whole).max()
            want = whole if kind == "ibm" else ysum
            v = tc.judge_wave(f"{p.name} oracle {kind}: the speakers' sum", np.sum(outs, axis=0, dtype=np.float64),
                              want, want, np.sum(each, axis=0), hop)
            lines.append(v.line())
            fails += v.failures
    print("\n".join(lines))
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------- 5. determinism
def test_an_utterance_has_the_same_bits_alone_and_in_any_batch(ctxs):
    """The 4133-sample utterance alone and as member 3 of a ragged batch of five, every mode; int16
    input against its float32 twin."""
    def variant(n, seed, K):
        return tc.noise_pairs(K, ((n, False),), seed)[0]

    for K in (2, 3):
        me = variant(4133, tc.ORACLE_SEED, K)
        batch = [variant(900, 1, K), variant(6000, 2, K), variant(512, 3, K), me, variant(2500, 4, K)]
        c = ctxs(me.geo)
        if K == 2:
            for kind in tc.KINDS:
                alone, st1, _ = mask_batch(c, kind, [me], 2.0)
                among, st5, _ = mask_batch(c, kind, batch, 2.0)
                twin, st16, _ = mask_batch(c, kind, [me], 2.0, pcm=True)
                assert np.array_equal(alone[0], among[3], equal_nan=True), kind
                assert np.array_equal(alone[0], twin[0], equal_nan=True), kind
                assert st1[0] == st5[3] == st16[0], kind
            masks = [given_mask(p, 3 + i) for i, p in enumerate(batch)]
            refs = [bool(i % 2) for i in range(5)]
            norm = [0.5] * 5
            for r in (None, refs):
                alone, _ = separate(c, [me], [masks[3]], None if r is None else [r[3]], norm[:1])
                among, _ = separate(c, batch, masks, r, norm)
                twin, _ = separate(c, [me], [masks[3]], None if r is None else [r[3]], norm[:1], pcm=True)
                assert np.array_equal(alone[0], among[3])
                assert np.array_equal(alone[0], twin[0])
        for kind in tc.ORACLE_KINDS:
            alone, _ = oracle(c, kind, [me])
            among, _ = oracle(c, kind, batch)
            twin, _ = oracle(c, kind, [me], pcm=True)
            for k in range(K):
                assert np.array_equal(alone[k], among[3 * K + k]), (kind, k)
                assert np.array_equal(alone[k], twin[k]), (kind, k)


# ---------------------------------------------------------------- 6. the fused path against the chain
def test_fused_path_against_the_stand_alone_chain(ctxs):
    """setk_stft -> setk_tf_mask / setk_tf_apply -> setk_istft against the fused entries.  Both are
    judged by the cell measure in the tests above (the chain's mask here); whether they agree bit
    for bit is printed and recorded in PARITY_NOTES_TFMASK.md."""
    fails, lines = [], []
    for p in pairs("noise_pairs"):
        c = ctxs(p.geo)
        T = p.T
        St = np.empty((1, T, F), np.complex64)
        Sm = np.empty((1, T, F), np.complex64)
        c.stft(p.tgt[None], St)
        c.stft(p.mix[None], Sm)
        for kind in tc.KINDS:
            chain = np.empty((T, width(kind)), np.float32)
            c.tf_mask(kind, St[0], Sm[0], T, F, chain, cutoff=2.0, want_stats=False)
            fused = mask_batch(c, kind, [p], 2.0)[0][0]
            same = np.array_equal(chain, fused, equal_nan=True)
            with np.errstate(all="ignore"):
                lines.append(f"{p.name}:{kind}: chain and fused {'agree bit for bit' if same else 'differ'}"
                             f" (max |d| {np.nanmax(np.abs(chain - fused)):.3e})")
            v = tc.judge_mask(f"{p.name}:{kind} (chain)", kind, chain, p, 2.0)
            fails += v.failures
        mk = given_mask(p, 11)
        enh = np.empty((1, T, F), np.complex64)
        c.tf_apply(Sm[0], mk, T, F, enh[0])
        wav = np.empty((1, c.istft_num_samples(T)), np.float32)
        c.istft(enh, 1, T, None, None, wav)
        fused = separate(c, [p], [mk])[0][0]
        lines.append(f"{p.name}: separation chain and fused "
                     f"{'agree bit for bit' if np.array_equal(wav[0], fused) else 'differ'}"
                     f" (max |d| {np.abs(wav[0] - fused).max():.3e})")
        y, y32, inp = tc.wave_reference(p, [mk])[0]
        fails += tc.judge_wave(f"{p.name} separation (chain)", wav[0], y, y32, inp, p.geo.hop).failures
    print("\n".join(lines))
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------- the operator path
@pytest.mark.parametrize("which", [0, 1])
def test_other_transform_sizes_take_the_operator_path(which):
    """frame_len 400 in n_fft 512 and n_fft 256 through the engines."""
    from setk_amd.engine import BatchMaskComputer, BatchMaskSeparator, BatchOracleSeparator
    p = pairs("other_size_pairs")[which]
    g = p.geo
    kw = dict(frame_len=g.frame_len, frame_hop=g.hop, center=g.center, round_power_of_two=True, window="hann")
    fails = []
    for kind in tc.KINDS:
        e = BatchMaskComputer(kind, cutoff=2.0, **kw)
        got = e.run([(p.tgt, p.mix)])[0]
        e.close()
        fails += tc.judge_mask(f"{p.name}:{kind} (engine)", kind, got, p, 2.0).failures
    mk = (1.2 * np.random.default_rng(5).random((p.T, g.F))).astype(np.float32)
    e = BatchMaskSeparator(**kw)
    got = e.run([p.mix], [mk.T if which else mk])[0]       # (an F x T mask is transposed)
    e.close()
    y, y32, inp = tc.wave_reference(p, [mk], norm=float(np.abs(p.mix).max()))[0]       # (mixed_norm is the default)
    fails += tc.judge_wave(f"{p.name} separation (engine)", got, y, y32, inp, g.hop).failures
    e = BatchOracleSeparator("irm", **kw)
    outs = e.run([(p.mix, p.targets)])[0]
    e.close()
    ts, m = p.spectra()
    masks = [np.asarray(x, np.float64) for x in tc.oracle_formula("irm", m, ts)]
    refs = tc.wave_reference(p, masks, a_mask=[tc.oracle_wave_extra("irm", p, k, masks[k]) for k in range(2)])
    for k in range(2):
        fails += tc.judge_wave(f"{p.name} oracle irm {k} (engine)", outs[k], *refs[k], g.hop).failures
    assert not fails, "\n".join(fails[:20])


# ---------------------------------------------------------------- 7. refusals
def test_refusals(ctxs, tmp_path):
    from setk_amd import _ffi
    from setk_amd.engine import BatchMaskComputer, BatchOracleSeparator
    p = pairs("noise_pairs")[2]
    c = ctxs(p.geo)
    wide = tc.noise_pairs(9, ((4133, False),))[0]
    with pytest.raises(_ffi.SetkUnsupported, match="at most 8 targets"):
        oracle(c, "irm", [wide])
    for kind in ("psa", "crm"):
        with pytest.raises(ValueError, match="ibm, irm, iam or psm"):
            oracle(c, kind, [p])
    with pytest.raises(ValueError, match="unknown mask"):
        mask_batch(c, "smm", [p], -1.0)
    with pytest.raises(ValueError, match="different length"):
        BatchMaskComputer("irm", center=False).run([(p.tgt[:-1], p.mix)])
    with pytest.raises(ValueError, match="different length"):
        BatchOracleSeparator("irm", center=False).run([(p.mix, [p.targets[0], p.targets[1][:-3]])])
    other = new_ctx(sc.Geom(n_fft=256, hop=128))
    try:
        with pytest.raises(_ffi.SetkUnsupported, match="n_fft = 512"):
            mask_batch(other, "irm", [tc.noise_pairs(2, ((4133, True),))[0]], -1.0)
    finally:
        other.close()
    from setk_amd.sptk import compute_mask as cli
    for name in ("a", "b"):
        (tmp_path / f"{name}.scp").write_text("")
    with pytest.raises(_ffi.SetkUnsupported, match="exraw"):
        cli.main([str(tmp_path / "a.scp"), str(tmp_path / "b.scp"), str(tmp_path / "m.ark"), "--format", "exraw"])


# ---------------------------------------------------------------- 8. the command lines
def test_command_lines_end_to_end(tmp_path):
    """Three short wav pairs written here, the three tools in child processes: archive keys, shapes
    and values against the goldens of the reference tools (ref_tfmask.npz), wav files to the PCM16
    floor."""
    import scipy.io.wavfile
    from setk_amd.libs.data_handler import ScriptReader
    gold = np.load(tc.GOLDEN)
    keys = [str(k) for k in gold["cli_keys"]]
    scps = {}
    for role in ("clean", "other", "noisy"):
        with open(tmp_path / f"{role}.scp", "w") as fd:
            for k in keys:
                path = tmp_path / f"{role}_{k}.wav"
                scipy.io.wavfile.write(path, 16000, gold[f"cli_{role}_{k}"])
                fd.write(f"{k} {path}\n")
        scps[role] = str(tmp_path / f"{role}.scp")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def tool(name, *args):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "sptk", f"{name}.py"), *args],
                           capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout + r.stderr

    pairs_of = {k: tc.Pair(k, [gold[f"cli_clean_{k}"].astype(np.float32) / np.float32(32768)],
                           gold[f"cli_noisy_{k}"].astype(np.float32) / np.float32(32768), sc.Geom())
                for k in keys}
    fails = []
    for kind, cutoff in (("irm", -1.0), ("psm", 2.0), ("crm", -1.0)):
        ark, scp = str(tmp_path / f"{kind}.ark"), str(tmp_path / f"{kind}.scp")
        log = tool("compute_mask", scps["clean"], scps["noisy"], ark, "--scp", scp, "--mask", kind,
                   "--cutoff", str(cutoff))
        rd = ScriptReader(scp)
        assert sorted(rd.index_keys) == sorted(keys)
        got = {k: rd[k] for k in keys}
        if kind == "psm":
            assert "items below zero" in log and "items over 2.00" in log
        for k in keys:
            want = gold[f"cli_{kind}_{k}"]
            assert got[k].shape == want.shape and got[k].dtype == np.float32, (kind, k, got[k].shape, want.shape)
            # the golden is the reference tool's float32 mask: both answer to the float64 reference
            fails += tc.judge_mask(f"cli {kind} {k}", kind, got[k], pairs_of[k], cutoff).failures
            fails += tc.judge_mask(f"golden {kind} {k}", kind, want, pairs_of[k], cutoff).failures
    # wav_separate with the irm archive, oracle_separate with two references
    tool("wav_separate", scps["noisy"], str(tmp_path / "irm.scp"), str(tmp_path / "sep"))
    tool("oracle_separate", scps["noisy"], "--ref-scp", scps["clean"] + "," + scps["other"], "--dump-dir",
         str(tmp_path / "ora"), "--mask", "irm")
    for k in keys:
        for path, name in ((tmp_path / "sep" / f"{k}.wav", f"cli_sep_{k}"),
                           (tmp_path / "ora" / "spk1" / f"{k}.wav", f"cli_ora1_{k}"),
                           (tmp_path / "ora" / "spk2" / f"{k}.wav", f"cli_ora2_{k}")):
            sr, w = scipy.io.wavfile.read(path)
            want = gold[name]
            assert sr == 16000 and w.dtype == np.int16 and w.shape == want.shape, (name, w.shape, want.shape)
            # the PCM16 floor: one step of rounding on either side of a float32 result
            assert np.abs(w.astype(np.int32) - want.astype(np.int32)).max() <= 2, name
    assert not fails, "\n".join(fails[:20])
