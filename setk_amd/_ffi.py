"""
ctypes binding of libsetk_hip.so (include/setk_hip.h).

There is no CPU fallback: if the HIP library has not been built or no GPU is
visible, every operator raises.  PyTorch is imported first so that its bundled
HIP runtime (same SONAME, libamdhip64.so.7) is the one the library binds to --
torch tensors and this library then share one runtime, one device context and
torch's streams.  A process that needs none of that (the streaming CLI: buffers,
streams and events come from the library itself) sets TORCH_FREE and skips the import.

The file follows the header: per feature its constants, structure, builder and the entries of
PROTOTYPES (tests/test_ffi_header.py holds all of them to the header), then the loader, then
Context with its methods in the same order.
"""
import ctypes
import os
import re
import sys
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SETK_LIB", os.path.join(_HERE, "libsetk_hip.so"))

# Every function of the header, in its order: name -> (return type, argument types).
PROTOTYPES = {}
I, Z = c_int, c_size_t
H = c_void_p           # setk_handle_t / setk_comm_t
P = c_void_p           # a data pointer, host or device (also where the header says int*: status, index)
S = c_void_p           # the hipStream_t
PP = POINTER(c_void_p)  # a host table of data pointers
IP = POINTER(c_int)     # a host array of int

SETK_OK = 0
ERR_INVALID, ERR_UNSUPPORTED, ERR_HIP, ERR_NOMEM = -1, -2, -3, -4
NUM_OK, NUM_SINGULAR, NUM_NOCONV, NUM_NONFINITE = 0, 1, 2, 3
NUM_RANKDEF = 4  # WPE: rank-deficient tap correlation, columns dropped -- a note, not an error
BF_MVDR, BF_GEVD, BF_PMWF, BF_MPDR, BF_MPDR_WHITEN = 0, 1, 2, 3, 4
RANK1_NONE, RANK1_EIG, RANK1_GEV = 0, 1, 2
FLAG_BAN, FLAG_CLAMP_MASK, FLAG_POST_MASK, FLAG_NO_GAUGE, FLAG_OUT_PCM16 = 1, 2, 4, 8, 16
FLAG_NO_RENORM = 32
FLAG_STRICT_REFERENCE = 64  # numpy.linalg.solve's exact-zero-pivot refusals (setk_hip.h)
FLAG_IN_PCM16 = 128  # enhance_batch: audio[u] is planar int16 [C][pcm16_channel_stride(N)]


class BfOpts(ctypes.Structure):
    _fields_ = [("kind", c_int), ("flags", c_int), ("pmwf_beta", c_float),
                ("pmwf_ref", c_int), ("rank1", c_int)]


# ---- lifetime; host-memory plumbing; buffers, streams, events; the STFT plan ----
PROTOTYPES.update(
    setk_abi_version=(I, []),
    setk_create=(I, [POINTER(H), I]),
    setk_destroy=(I, [H]),
    setk_last_error=(c_char_p, [H]),
    setk_device_pci_bus_id=(I, [H, c_char_p, I]),
    setk_host_register=(I, [H, P, Z]),
    setk_host_unregister=(I, [H, P]),
    setk_memcpy_h2d_async=(I, [H, P, P, Z, S]),
    setk_memcpy_d2h_async=(I, [H, P, P, Z, S]),
    setk_device_alloc=(I, [H, Z, PP]),
    setk_device_free=(I, [H, P]),
    setk_host_alloc=(I, [H, Z, PP]),
    setk_host_free=(I, [H, P]),
    setk_host_read_payloads=(I, [I, POINTER(c_char_p), POINTER(c_longlong), POINTER(c_longlong), PP, I,
                                 c_longlong, IP]),
    setk_stream_create=(I, [H, PP]),
    setk_stream_destroy=(I, [H, S]),
    setk_stream_synchronize=(I, [H, S]),
    setk_stream_wait_event=(I, [H, S, P]),
    setk_event_create=(I, [H, PP]),
    setk_event_destroy=(I, [H, P]),
    setk_event_record=(I, [H, P, S]),
    setk_event_synchronize=(I, [H, P]),
    setk_stft_plan=(I, [H, I, I, I, I, P]),
    setk_stft_num_frames=(I, [H, I]),
    setk_istft_num_samples=(I, [H, I, I]),
)


def host_read_payloads(paths, offsets, nbytes, dsts, threads, mmap_min_bytes):
    """setk_host_read_payloads: payload i = nbytes[i] bytes at offsets[i] of paths[i] -> address
    dsts[i], by the library's pool of native reader threads.  Returns the list of errno values
    (0: read).  No handle, no device: the call releases the interpreter lock for the whole batch."""
    n = len(paths)
    if not n:
        return []
    lib = load_library()
    files = (c_char_p * n)(*[os.fsencode(p) for p in paths])
    at = (c_longlong * n)(*[int(v) for v in offsets])
    size = (c_longlong * n)(*[int(v) for v in nbytes])
    status = _ints((), n)
    rc = lib.setk_host_read_payloads(n, files, at, size, _ptrs([int(v) for v in dsts], n), int(threads),
                                     int(mmap_min_bytes), status)
    if rc != 0:
        raise SetkError(f"setk_host_read_payloads: bad arguments ({rc})")
    return list(status)


# ---- modular operators ----
KALDI_KINDS = {"CM": 1, "CM2": 2, "CM3": 3}  # SETK_KALDI_*

PROTOTYPES.update(
    setk_stft=(I, [H, P, I, I, P, S]),
    setk_stft_batch=(I, [H, I, I, PP, IP, PP, I, S]),
    setk_istft=(I, [H, P, I, I, I, P, P, S]),
    setk_covar=(I, [H, P, P, I, I, I, P, S]),
    setk_pevd=(I, [H, P, P, I, I, I, P, P, S]),
    setk_weights=(I, [H, POINTER(BfOpts), P, P, P, I, I, P, P, IP, S]),
    setk_pcm16_to_float=(I, [H, P, I, I, P, S]),
    setk_pcm16_to_float_batch=(I, [H, I, I, PP, IP, PP, P, S]),
    setk_pcm16_channel_stride=(I, [I]),
    setk_pcm16_deinterleave_batch=(I, [H, I, I, PP, IP, PP, P, S]),
    setk_kaldi_cm_decode_batch=(I, [H, I, IP, POINTER(c_float), POINTER(c_float), IP, IP, IP, PP, PP, S]),
    setk_float_to_pcm16=(I, [H, P, I, I, P, S]),
    setk_ban=(I, [H, P, P, I, I, P, S]),
    setk_rank1=(I, [H, P, P, I, I, P, P, S]),
    setk_beamform=(I, [H, P, P, I, I, I, P, S]),
)

# ---- CGMM and CACGMM mask estimation ----
CGMM_UPDATE_ALPHA = 1
CACGMM_UPDATE_ALPHA = 1
CACGMM_CGMM_INIT = 2

PROTOTYPES.update(
    setk_cgmm_masks=(I, [H, P, I, I, I, I, P, P, P, I, S]),
    setk_cgmm_masks_k=(I, [H, P, I, I, I, I, I, P, P, P, I, S]),
    setk_cgmm_masks_k_status=(I, [H, P, I, I, I, I, I, P, P, P, I, P, S]),
    setk_cgmm_masks_batch=(I, [H, I, I, PP, IP, I, I, PP, PP, I, I, S]),
    setk_cgmm_estimate_batch=(I, [H, I, I, PP, IP, I, PP, PP, I, S]),
    setk_cgmm_bin_config=(I, [I, I, IP]),
    setk_cacgmm_masks=(I, [H, P, I, I, I, I, I, P, I, P, P, S]),
    setk_cacgmm_estimate_batch=(I, [H, I, I, PP, IP, I, I, PP, I, PP, IP, S]),
)


def cgmm_bin_config(num_channels, max_frames):
    """setk_cgmm_bin_config: (index, threads, frames per thread, of them in registers) of the
    bin-resident EM configuration the two-class CGMM entries run for this channel count and
    longest utterance; (-1, 0, 0, 0) when they run the streaming kernels.  No handle, no device."""
    info = (c_int * 3)()
    idx = load_library().setk_cgmm_bin_config(int(num_channels), int(max_frames), info)
    return (idx, info[0], info[1], info[2]) if idx >= 0 else (-1, 0, 0, 0)


def cacgmm_flags(update_alpha, cgmm_init):
    return (CACGMM_UPDATE_ALPHA if update_alpha else 0) | (CACGMM_CGMM_INIT if cgmm_init else 0)


# ---- directional features, fixed beamformer, WPE, AuxIVA ----
PROTOTYPES.update(
    setk_directional_feats=(I, [H, P, P, IP, I, I, I, I, P, S]),
    setk_apply_weights_batch=(I, [H, I, I, PP, IP, P, I, IP, PP, I, S]),
    setk_wpe=(I, [H, P, I, I, I, I, I, I, I, P, P, P, P, S]),
    setk_wpe_step=(I, [H, P, I, I, I, I, I, P, P, P, S]),
    setk_wpe_batch=(I, [H, I, PP, I, IP, I, I, I, I, I, PP, P, S]),
    setk_wpe_batch_var=(I, [H, I, PP, I, IP, I, I, I, I, I, PP, PP, PP, P, S]),
    setk_wpe_batch_fnt=(I, [H, I, PP, I, IP, I, I, I, I, I, PP, P, S]),
    setk_wpe_form=(I, [I, I, IP, IP, IP]),
    setk_auxiva=(I, [H, P, I, I, I, I, P, P, S]),
    setk_auxiva_batch=(I, [H, I, I, PP, IP, I, PP, P, I, S]),
)


def wpe_failed(status):
    """Boolean array: the bins whose WPE status is an error (SETK_NUM_RANKDEF is only a note)."""
    st = np.asarray(status)
    return (st != NUM_OK) & (st != NUM_RANKDEF)


def wpe_form(num_channels, taps):
    """setk_wpe_form: (wide, tiles per wavefront, frames per staged chunk) of the step kernel the
    WPE entries launch for this shape; None for a shape they refuse.  No handle, no device."""
    w, n, tc = c_int(), c_int(), c_int()
    rc = load_library().setk_wpe_form(int(num_channels), int(taps), ctypes.byref(w), ctypes.byref(n),
                                      ctypes.byref(tc))
    return (bool(w.value), n.value, tc.value) if rc == SETK_OK else None


# ---- sound source localisation ----
SSL_BACKENDS = {"ml": 0, "srp": 1, "music": 2}  # SETK_SSL_*


class SslOpts(ctypes.Structure):
    _fields_ = [("backend", c_int), ("n_pairs", c_int), ("pairs", POINTER(c_int)),
                ("compression", c_float), ("norm", c_int), ("eps", c_double)]


def ssl_opts(backend, srp_pair=None, compression=0.0, eps=1e-8, norm=False):
    """setk_ssl_opts for a backend name; srp_pair is the reference's (left indices, right
    indices).  The returned structure keeps its pair table alive."""
    o = SslOpts(backend=SSL_BACKENDS[backend], n_pairs=0, pairs=None, compression=float(compression),
                norm=1 if norm else 0, eps=float(eps))
    if backend == "srp":
        if srp_pair is None:
            raise ValueError("srp_pair cannot be None, (list, list)")
        left, right = srp_pair
        if len(left) != len(right) or not len(left):
            raise ValueError("srp_pair: two index lists of the same, non-zero length")
        o._pairs = _ints([v for lr in zip(left, right) for v in lr])
        o.pairs = ctypes.cast(o._pairs, POINTER(c_int))
        o.n_pairs = len(left)
    return o


PROTOTYPES.update(
    setk_ssl_scores=(I, [H, POINTER(SslOpts), P, P, P, I, I, I, I, IP, I, P, P, P, S]),
    setk_ssl_batch=(I, [H, POINTER(SslOpts), I, I, PP, IP, PP, P, I, IP, IP, P, P, P, S]),
)

# ---- geometry-driven spatial features ----
SPATIAL_KINDS = {"ipd": 0, "cos_ipd": 1, "cos_sin_ipd": 2, "df": 3, "srp": 4}  # SETK_SPATIAL_*


class SpatialOpts(ctypes.Structure):
    _fields_ = [("kind", c_int), ("n_pairs", c_int), ("pairs", POINTER(c_int)), ("num_doas", c_int),
                ("table", c_void_p), ("pair_weight", POINTER(c_float)), ("num_sv", c_int),
                ("steer_vector", c_void_p), ("n_index", c_int), ("doa_index", POINTER(c_int))]


def spatial_dpad(num_doas):
    """Row pitch of the SRP table: the directions rounded up to a multiple of 64."""
    return (int(num_doas) + 63) & ~63


def spatial_opts(kind, pairs, table=None, num_doas=0, pair_weight=None, steer_vector=None, num_sv=0,
                 doa_index=None):
    """setk_spatial_opts for a kind name.  pairs [(l, r), ...]; SRP: table [P][F][spatial_dpad(D)]
    complex64 (numpy array or device address) and the weight of every pair; DF: steer_vector
    [A][C][F] complex64 (numpy array or device address) and doa_index, one list of directions per
    utterance (all of one length).  The returned structure keeps its host tables alive."""
    o = SpatialOpts(kind=SPATIAL_KINDS[kind])
    o._pairs = _ints([v for p in pairs for v in p])
    o.pairs = ctypes.cast(o._pairs, POINTER(c_int))
    o.n_pairs = len(o._pairs) // 2
    if kind == "srp":
        o._table = table
        o.table = _ptr(table)
        o.num_doas = int(num_doas)
        o._weight = (c_float * o.n_pairs)(*[float(w) for w in pair_weight])
        o.pair_weight = ctypes.cast(o._weight, POINTER(c_float))
    elif kind == "df":
        o._sv = steer_vector
        o.steer_vector = _ptr(steer_vector)
        o.num_sv = int(num_sv)
        idx = [[int(v) for v in row] for row in doa_index]
        if len({len(row) for row in idx}) != 1 or not idx[0]:
            raise ValueError("doa_index: the same, non-zero number of directions for every utterance")
        o.n_index = len(idx[0])
        o._index = _ints([v for row in idx for v in row])
        o.doa_index = ctypes.cast(o._index, POINTER(c_int))
    return o


def spatial_width(opts, F):
    """Columns of the feature map of one utterance."""
    if opts.kind == SPATIAL_KINDS["srp"]:
        return opts.num_doas
    if opts.kind == SPATIAL_KINDS["df"]:
        return opts.n_index * F
    return (2 if opts.kind == SPATIAL_KINDS["cos_sin_ipd"] else 1) * opts.n_pairs * F


PROTOTYPES.update(
    setk_spatial_feats=(I, [H, POINTER(SpatialOpts), P, I, I, I, P, S]),
    setk_spatial_batch=(I, [H, POINTER(SpatialOpts), I, I, PP, IP, I, PP, S]),
)

# ---- OM-LSA noise suppression ----
NS_KINDS = {"mcra": 0, "imcra": 1}  # SETK_NS_*
NS_OUT_GAIN = 1
NS_OUT_SPEC = 2
NS_MAX_TAPS = 63


class NsOpts(ctypes.Structure):
    _fields_ = [("kind", c_int), ("flags", c_int), ("alpha", c_double), ("alpha_s", c_double),
                ("alpha_d", c_double), ("gmin", c_double), ("xi_min", c_double),
                ("n_mcra", c_int), ("n_local", c_int), ("n_global", c_int),
                ("w_mcra", POINTER(c_double)), ("w_local", POINTER(c_double)), ("w_global", POINTER(c_double)),
                ("delta", c_double), ("beta", c_double), ("alpha_p", c_double),
                ("q_max", c_double), ("zeta_min", c_double), ("zeta_max", c_double),
                ("zeta_p_min", c_double), ("zeta_p_max", c_double), ("L", c_int), ("M", c_int),
                ("inv_b_min", c_double), ("gamma0", c_double), ("gamma1", c_double),
                ("zeta0", c_double), ("V", c_int), ("U", c_int), ("eps", c_double)]


def ns_opts(kind, eps=1e-7, gain=True, spec=False, w_mcra=None, w_local=None, w_global=None, **values):
    """setk_ns_opts for a kind name ("mcra" / "imcra"): the windows as float64 tap arrays, every
    other field of the structure by its name.  The returned structure keeps its taps alive."""
    o = NsOpts(kind=NS_KINDS[kind], flags=(NS_OUT_GAIN if gain else 0) | (NS_OUT_SPEC if spec else 0),
               eps=float(eps))
    for name, w in (("mcra", w_mcra), ("local", w_local), ("global", w_global)):
        if w is None:
            continue
        w = [float(v) for v in w]
        keep = (c_double * len(w))(*w)
        setattr(o, "_w_" + name, keep)
        setattr(o, "w_" + name, ctypes.cast(keep, POINTER(c_double)))
        setattr(o, "n_" + name, len(w))
    known = {f[0] for f in NsOpts._fields_}
    for name, v in values.items():
        if name not in known:
            raise TypeError(f"setk_ns_opts has no field {name}")
        setattr(o, name, v)
    return o


PROTOTYPES.update(
    setk_ns_gain=(I, [H, POINTER(NsOpts), P, I, I, P, P, P, S]),
    setk_ns_batch=(I, [H, POINTER(NsOpts), I, PP, IP, PP, PP, P, I, S]),
    setk_expint_e1=(I, [H, P, P, I, S]),
)

# ---- oracle TF masks and mask-based separation ----
TFMASK_IBM, TFMASK_IRM, TFMASK_IAM, TFMASK_PSM, TFMASK_PSA, TFMASK_CRM = range(6)
TFMASK_MAX_TARGETS = 8
TFMASK_NAMES = {"ibm": TFMASK_IBM, "irm": TFMASK_IRM, "iam": TFMASK_IAM, "psm": TFMASK_PSM, "psa": TFMASK_PSA,
                "crm": TFMASK_CRM}
ORACLE_MASKS = ("iam", "irm", "ibm", "psm")  # oracle_separate.py's choices


class TfmaskStats(ctypes.Structure):
    """setk_tfmask_stats: what compute_mask.py logs for one mask."""
    _fields_ = [("over", ctypes.c_longlong), ("below", ctypes.c_longlong), ("below_sum", c_double)]


def tfmask_kind(name):
    try:
        return TFMASK_NAMES[name]
    except KeyError:
        raise ValueError(f"unknown mask {name!r}: one of {sorted(TFMASK_NAMES)}") from None


PROTOTYPES.update(
    setk_tf_mask=(I, [H, I, P, P, I, I, c_float, P, P, S]),
    setk_tf_apply=(I, [H, P, P, P, I, I, P, S]),
    setk_tf_mask_batch=(I, [H, I, I, PP, PP, IP, c_float, PP, P, P, I, S]),
    setk_tf_separate_batch=(I, [H, I, PP, PP, IP, PP, P, IP, PP, P, I, S]),
    setk_oracle_separate_batch=(I, [H, I, I, I, PP, PP, IP, IP, PP, P, I, S]),
)

# ---- SI-SNR scoring ----
FLAG_KEEP_DC = 256  # si_snr(remove_dc=False)
METRIC_MAX_SOURCES = 8  # the search walks K! orders

PROTOTYPES.update(
    setk_si_snr_batch=(I, [H, I, IP, PP, IP, PP, IP, IP, c_double, I, P, P, P, P, S]),
    setk_si_snr=(I, [H, P, P, I, c_double, I, P, S]),
)

# ---- data simulation ----
SIMU_MAX_TAPS, SIMU_MAX_CHANNELS = 16384, 16
SIMU_REPEAT = 1


class SimuSource(ctypes.Structure):
    _fields_ = [("audio", c_void_p), ("rir", c_void_p), ("num_samples", c_int), ("channels", c_int),
                ("rir_channels", c_int), ("rir_taps", c_int), ("begin", c_int), ("flags", c_int),
                ("snr", c_double)]


class SimuRecipe(ctypes.Structure):
    _fields_ = [("speakers", POINTER(SimuSource)), ("noises", POINTER(SimuSource)), ("n_speakers", c_int),
                ("n_noises", c_int), ("iso", c_void_p), ("iso_samples", c_int), ("iso_channels", c_int),
                ("iso_snr", c_double), ("dump_channel", c_int), ("pad_", c_int),
                ("norm_factor", c_double), ("mix", c_void_p), ("spk_ref", POINTER(c_void_p)),
                ("noise_ref", c_void_p)]


def simu_source(audio, num_samples, channels=1, rir=None, rir_channels=0, rir_taps=0, begin=0, snr=0.0,
                repeat=False):
    """setk_simu_source: audio / rir are device addresses (planar channels)."""
    return SimuSource(audio=audio, rir=rir, num_samples=int(num_samples), channels=int(channels),
                      rir_channels=int(rir_channels), rir_taps=int(rir_taps), begin=int(begin),
                      flags=SIMU_REPEAT if repeat else 0, snr=float(snr))


def simu_recipe(speakers, noises=(), iso=None, iso_samples=0, iso_channels=0, iso_snr=0.0, dump_channel=-1,
                norm_factor=0.9):
    """setk_simu_recipe over lists of simu_source; the outputs (mix, spk_ref, noise_ref) are set with
    simu_recipe_outputs once the caller knows the sizes.  The structure keeps its tables alive."""
    r = SimuRecipe(n_speakers=len(speakers), n_noises=len(noises), iso=iso, iso_samples=int(iso_samples),
                   iso_channels=int(iso_channels), iso_snr=float(iso_snr), dump_channel=int(dump_channel),
                   norm_factor=float(norm_factor))
    r._speakers = (SimuSource * max(len(speakers), 1))(*speakers)
    r.speakers = ctypes.cast(r._speakers, POINTER(SimuSource))
    if len(noises):
        r._noises = (SimuSource * len(noises))(*noises)
        r.noises = ctypes.cast(r._noises, POINTER(SimuSource))
    r._refs = _ptrs((), max(len(speakers), 1))
    r.spk_ref = ctypes.cast(r._refs, POINTER(c_void_p))
    return r


def simu_recipe_outputs(r, mix, spk_refs, noise_ref=None):
    r.mix = mix
    for i, p in enumerate(spk_refs):
        r._refs[i] = p
    r.noise_ref = noise_ref


def simu_shape(r):
    """(channels N, samples L) of a recipe's mixture; no handle, no device."""
    lib = load_library()
    N, L = lib.setk_simu_num_channels(ctypes.byref(r)), lib.setk_simu_num_samples(ctypes.byref(r))
    if N < 0 or L < 0:
        raise ValueError("a recipe needs at least one speaker")
    return N, L


PROTOTYPES.update(
    setk_fir_reverb=(I, [H, P, I, P, I, I, P, P, I, S]),
    setk_simu_num_samples=(I, [POINTER(SimuRecipe)]),
    setk_simu_num_channels=(I, [POINTER(SimuRecipe)]),
    setk_simu_batch=(I, [H, I, POINTER(SimuRecipe), P, I, S]),
)

# ---- room impulse responses by the image method ----
RIR_MAX_TAPS, RIR_MAX_MICS = 16384, 16
RIR_MIC_BIDIRECTIONAL, RIR_MIC_HYPERCARDIOID, RIR_MIC_CARDIOID, RIR_MIC_SUBCARDIOID = 0, 1, 2, 3
RIR_MIC_OMNIDIRECTIONAL = 4
RIR_MIC_TYPES = {"bidirectional": 0, "hypercardioid": 1, "cardioid": 2, "subcardioid": 3, "omnidirectional": 4}
RIR_NO_SPLIT = 1  # one workgroup walks all images of a (RIR, microphone) pair


class RirSpec(ctypes.Structure):
    _fields_ = [("room", POINTER(c_float)), ("source", POINTER(c_float)), ("mics", POINTER(c_float)),
                ("beta", POINTER(c_float)), ("angle", POINTER(c_float)), ("n_mics", c_int), ("n_beta", c_int),
                ("mic_type", c_int), ("order", c_int), ("num_samples", c_int), ("hp_filter", c_int),
                ("samp_frequency", c_float), ("sound_velocity", c_float)]


def rir_spec(room, source, mics, beta, num_samples, samp_frequency=16000.0, sound_velocity=340.0, order=-1,
             hp_filter=True, mic_type="omnidirectional", angle=None):
    """setk_rir_spec over float32 copies of the arrays (the structure keeps them alive): room and
    source 3 values, mics n x 3, beta the reflection coefficients (six; any other count is passed on
    for the library to refuse), angle None or (azimuth, elevation)."""
    if mic_type not in RIR_MIC_TYPES:
        raise ValueError(f"Unknown option values: --microphone-type={mic_type}")
    mics = np.ascontiguousarray(mics, dtype=np.float32).reshape(-1, 3)
    keep = dict(room=np.ascontiguousarray(room, dtype=np.float32).reshape(3),
                source=np.ascontiguousarray(source, dtype=np.float32).reshape(3), mics=mics,
                beta=np.ascontiguousarray(beta, dtype=np.float32).reshape(-1))
    if angle is not None:
        keep["angle"] = np.ascontiguousarray(angle, dtype=np.float32).reshape(2)
    sp = RirSpec(n_mics=mics.shape[0], n_beta=keep["beta"].size, mic_type=RIR_MIC_TYPES[mic_type], order=int(order),
                 num_samples=int(num_samples), hp_filter=1 if hp_filter else 0,
                 samp_frequency=float(samp_frequency), sound_velocity=float(sound_velocity))
    for name, a in keep.items():
        setattr(sp, name, a.ctypes.data_as(POINTER(c_float)))
    sp._keep = keep
    return sp


PROTOTYPES.update(
    setk_rir_generate_batch=(I, [H, I, POINTER(RirSpec), PP, P, I, S]),
    setk_rir_generate=(I, [H, POINTER(RirSpec), P, P, I, S]),
)


# ---- fused hot path; the RCCL barrier; stage timings ----
class BatchTaps(ctypes.Structure):
    _fields_ = [("Rs", c_void_p), ("Rn", c_void_p), ("weight", c_void_p), ("maxabs", c_void_p)]


class OnlineOpts(ctypes.Structure):
    _fields_ = [("chunk_size", c_int), ("alpha", c_float)]


class OnlineTaps(ctypes.Structure):
    _fields_ = [("Rs", c_void_p), ("Rn", c_void_p), ("weight", c_void_p)]


PROTOTYPES.update(
    setk_enhance_batch=(I, [H, POINTER(BfOpts), I, I, PP, IP, PP, PP, PP, IP, S]),
    setk_enhance_batch_taps=(I, [H, POINTER(BfOpts), I, I, PP, IP, PP, PP, PP, IP, POINTER(BatchTaps), S]),
    setk_online_num_chunks=(I, [H, I, I]),
    setk_enhance_online_batch=(I, [H, POINTER(BfOpts), POINTER(OnlineOpts), I, I, PP, IP, PP, PP, PP, IP,
                                   POINTER(OnlineTaps), S]),
    setk_comm_unique_id=(I, [c_char_p]),
    setk_comm_create=(I, [POINTER(H), I, c_char_p, I, I]),
    setk_comm_allreduce_f64=(I, [H, POINTER(c_double), I, I]),
    setk_comm_barrier=(I, [H]),
    setk_comm_destroy=(I, [H]),
    setk_comm_last_error=(c_char_p, []),
    setk_set_profiling=(I, [H, I]),
    setk_last_stage_ms=(I, [H, POINTER(c_float)]),
)


def exported_symbols():
    """Names declared in include/setk_hip.h (checked by the CPU test-suite)."""
    return list(PROTOTYPES)


# ---- the loader ----
class SetkError(RuntimeError):
    pass


class SetkUnsupported(SetkError, NotImplementedError):
    pass


_lib = None


# The streaming CLI needs no torch at all (buffers, streams and events come from the library):
# it sets this before the first Context so that the second of `import torch` is not spent.
# The library then runs on the HIP runtime of /opt/rocm; a process that is going to use torch
# tensors with this library must import torch BEFORE the library is loaded (the default).
TORCH_FREE = os.environ.get("SETK_TORCH_FREE", "") not in ("", "0")


def set_torch_free(ok=True):
    """What the CLIs call before the first Context: run torch-free unless the caller knows an
    input needs a torch path (`ok` false), the user said SETK_TORCH_FREE=0, or torch is loaded
    already.  Returns whether the process is torch-free now."""
    global TORCH_FREE
    if not ok or os.environ.get("SETK_TORCH_FREE", "") == "0" or "torch" in sys.modules:
        return TORCH_FREE and "torch" not in sys.modules
    TORCH_FREE = True
    return True


def import_torch(what="this path"):
    """torch for the code paths that run through torch tensors.  In a process that loaded the
    library torch-free the import would come too late (the library is bound to the HIP runtime
    of /opt/rocm by then; torch must be imported BEFORE it): say so instead of importing."""
    if TORCH_FREE and _lib is not None and "torch" not in sys.modules:
        raise SetkUnsupported(
            f"{what} runs through torch tensors, but this process loaded {LIB_PATH} torch-free "
            "(streaming CLI mode); re-run with SETK_TORCH_FREE=0")
    import torch
    return torch


def env_atoi(name, default):
    """An integer environment switch as the library's C side parses it (atoi: optional sign and
    leading digits, anything else is 0); `default` when the variable is unset."""
    v = os.environ.get(name)
    if v is None:
        return default
    m = re.match(r"\s*([+-]?\d+)", v)
    return int(m.group(1)) if m else 0


def load_library():
    """dlopen libsetk_hip.so and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SetkError(
            f"{LIB_PATH} is missing: build it with `python -m setk_amd.build` "
            "(there is no CPU fallback)")
    if not TORCH_FREE or "torch" in sys.modules:
        try:
            import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first)
        except Exception:  # pragma: no cover - torch is plumbing, not required
            pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    if hasattr(lib, "hoststub_report") and os.environ.get("SETK_ALLOW_HOSTSTUB") != "1":
        # tools/hoststub: the library linked against a host-memory stand-in for HIP whose
        # kernels do nothing -- test infrastructure for the host side, never a way to run
        raise SetkError(f"{LIB_PATH} is the test build against the HIP stand-in (tools/hoststub); "
                        "it computes nothing.  Tests that mean to load it set SETK_ALLOW_HOSTSTUB=1")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)  # (a library that lacks one of them does not load: AttributeError)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _ptr(x):
    """Raw address of a numpy array (host) or torch tensor (host/device)."""
    if x is None:
        return None
    if isinstance(x, int):  # a raw (device) address
        return x
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return x.ctypes.data
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr()
    raise TypeError(f"unsupported buffer type {type(x)}")


def _ptrs(items, n=None):
    """A host table of n (default: all) data pointers out of a list of addresses, arrays or
    tensors, entries that are missing or None being NULL; None for no list."""
    if items is None:
        return None
    table = c_void_p * (len(items) if n is None else n)
    try:
        return table(*items)  # plain addresses: the hot path's 3 x 125 of them stay out of _ptr
    except TypeError:
        return table(*[_ptr(x) for x in items])


def _ints(values, n=None):
    """A host array of n (default: all) int out of a list, entries that are missing being 0; None
    for no list."""
    if values is None:
        return None
    array = c_int * (len(values) if n is None else n)
    try:
        return array(*values)
    except TypeError:  # (a float among them)
        return array(*[int(v) for v in values])


def _torch():
    """torch, or None in a torch-free process (TORCH_FREE and nobody imported it)."""
    if TORCH_FREE and "torch" not in sys.modules:
        return None
    try:
        import torch
        return torch
    except Exception:  # pragma: no cover
        return None


def current_stream_ptr():
    """torch's current HIP stream as a raw hipStream_t (0 = default stream)."""
    torch = _torch()
    try:
        if torch is not None and torch.cuda.is_available():
            return torch.cuda.current_stream().cuda_stream
    except Exception:
        pass
    return 0


def _stream(stream):
    """The stream an operator runs on: the caller's, or torch's current one."""
    return current_stream_ptr() if stream is None else stream


class Context:
    """Owns one setk_handle_t (one GPU, one host thread at a time)."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._h = c_void_p()
        rc = self._lib.setk_create(ctypes.byref(self._h), int(device))
        if rc != SETK_OK:
            self._h = None
            raise SetkError(
                f"setk_create(device={device}) failed with {rc}: no usable MI355X / "
                "HIP runtime (the product path needs the GPU; there is no CPU fallback)")
        self.device = int(device)
        self.plan = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.setk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc == SETK_OK:
            return
        msg = self._lib.setk_last_error(self._h)
        msg = msg.decode() if msg else ""
        if rc == ERR_INVALID:
            raise ValueError(msg)
        if rc == ERR_UNSUPPORTED:
            raise SetkUnsupported(msg)
        raise SetkError(f"libsetk_hip error {rc}: {msg}")

    def _run(self, name, *args, stream=None):
        """The operator `name` on (handle, *args, the resolved stream), checked."""
        self.check(getattr(self._lib, name)(self._h, *args, _stream(stream)))

    def pci_bus_id(self):
        """PCI address of the handle's device ("0000:23:00.0"): the key to its NUMA node in
        sysfs (setk_amd/numa.py)."""
        buf = ctypes.create_string_buffer(32)
        self.check(self._lib.setk_device_pci_bus_id(self._h, buf, 32))
        return buf.value.decode().lower()

    # -- host-memory plumbing (thread safe) -----------------------------------
    def host_register(self, ptr, nbytes):
        """Pin [ptr, ptr + nbytes); returns False when the runtime refuses the range."""
        return self._lib.setk_host_register(self._h, c_void_p(int(ptr)), int(nbytes)) == SETK_OK

    def host_unregister(self, ptr):
        self._lib.setk_host_unregister(self._h, c_void_p(int(ptr)))

    def memcpy_h2d_async(self, dst, src, nbytes, stream):
        self.check(self._lib.setk_memcpy_h2d_async(self._h, c_void_p(int(dst)), c_void_p(int(src)),
                                                   int(nbytes), stream))

    def memcpy_d2h_async(self, dst, src, nbytes, stream):
        self.check(self._lib.setk_memcpy_d2h_async(self._h, c_void_p(dst), c_void_p(src),
                                                   ctypes.c_size_t(int(nbytes)), c_void_p(stream)))

    # -- buffers, streams, events (a host pipeline without a runtime binding of its own) ----
    def _out_ptr(self, fn, *args):
        p = c_void_p()
        self.check(fn(self._h, *args, ctypes.byref(p)))
        return p.value or 0

    def device_alloc(self, nbytes):
        return self._out_ptr(self._lib.setk_device_alloc, ctypes.c_size_t(int(nbytes)))

    def device_free(self, ptr):
        self.check(self._lib.setk_device_free(self._h, c_void_p(ptr)))

    def host_alloc(self, nbytes):
        """Page-locked host memory: (address, uint8 numpy view)."""
        nbytes = int(nbytes)
        addr = self._out_ptr(self._lib.setk_host_alloc, ctypes.c_size_t(nbytes))
        view = np.ctypeslib.as_array(ctypes.cast(addr, POINTER(ctypes.c_uint8)), shape=(nbytes,))
        return addr, view

    def host_free(self, addr):
        self.check(self._lib.setk_host_free(self._h, c_void_p(addr)))

    def stream_create(self):
        return self._out_ptr(self._lib.setk_stream_create)

    def stream_destroy(self, stream):
        self.check(self._lib.setk_stream_destroy(self._h, c_void_p(stream)))

    def stream_synchronize(self, stream):
        self.check(self._lib.setk_stream_synchronize(self._h, c_void_p(stream)))

    def stream_wait_event(self, stream, event):
        self.check(self._lib.setk_stream_wait_event(self._h, c_void_p(stream), c_void_p(event)))

    def event_create(self):
        return self._out_ptr(self._lib.setk_event_create)

    def event_destroy(self, event):
        self.check(self._lib.setk_event_destroy(self._h, c_void_p(event)))

    def event_record(self, event, stream):
        self.check(self._lib.setk_event_record(self._h, c_void_p(event), c_void_p(stream)))

    def event_synchronize(self, event):
        self.check(self._lib.setk_event_synchronize(self._h, c_void_p(event)))

    # -- plan ---------------------------------------------------------------
    def stft_plan(self, frame_len, frame_hop, n_fft, center, window=None):
        key = (int(frame_len), int(frame_hop), int(n_fft), bool(center),
               None if window is None else window.tobytes())
        if self.plan == key:
            return
        wp = None
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float32)
            if window.shape != (frame_len,):
                raise ValueError("window must have frame_len entries")
            wp = window.ctypes.data
        self.check(
            self._lib.setk_stft_plan(self._h, frame_len, frame_hop, n_fft,
                                     1 if center else 0, wp))
        self.plan = key

    def num_frames(self, num_samples):
        r = self._lib.setk_stft_num_frames(self._h, int(num_samples))
        if r < 0:
            self.check(r)
        return r

    def istft_num_samples(self, num_frames, nsamps=-1):
        r = self._lib.setk_istft_num_samples(self._h, int(num_frames),
                                             -1 if nsamps is None else int(nsamps))
        if r < 0:
            self.check(r)
        return r

    # -- modular operators (numpy in / numpy out, or device tensors) ---------
    def stft(self, audio, out, stream=None):
        C, N = audio.shape
        self._run("setk_stft", _ptr(audio), C, N, _ptr(out), stream=stream)

    def stft_batch(self, C, audio_ptrs, num_samples, spec_ptrs, stream=None, spec_pitch=0):
        """One launch for the spectrograms of a batch (device addresses)."""
        n = len(audio_ptrs)
        self._run("setk_stft_batch", n, int(C), _ptrs(audio_ptrs), _ints(num_samples, n), _ptrs(spec_ptrs, n),
                  int(spec_pitch), stream=stream)

    def istft(self, spec, batch, num_frames, nsamps, norm, out, stream=None):
        self._run("setk_istft", _ptr(spec), batch, num_frames, -1 if nsamps is None else int(nsamps), _ptr(norm),
                  _ptr(out), stream=stream)

    def covar(self, spec, mask, C, T, F, out, stream=None):
        self._run("setk_covar", _ptr(spec), _ptr(mask), C, T, F, _ptr(out), stream=stream)

    def pevd(self, Rs, Rn, F, C, flags, out, status, stream=None):
        self._run("setk_pevd", _ptr(Rs), _ptr(Rn), F, C, flags, _ptr(out), _ptr(status), stream=stream)

    def weights(self, opts, Rs, Rn, Ry, F, C, out, status, stream=None):
        ref = c_int(-1)
        self._run("setk_weights", ctypes.byref(opts), _ptr(Rs), _ptr(Rn), _ptr(Ry), F, C, _ptr(out), _ptr(status),
                  ctypes.byref(ref), stream=stream)
        return ref.value

    def pcm16_to_float(self, pcm, C, N, out, stream=None):
        """interleaved int16 frames pcm[N][C] -> float32 out[C][N] (= pcm / 32768)."""
        self._run("setk_pcm16_to_float", _ptr(pcm), C, N, _ptr(out), stream=stream)

    def _pcm16_batch(self, name, C, pcm_ptrs, num_samples, out_ptrs, power0, stream):
        n = len(pcm_ptrs)
        self._run(name, n, int(C), _ptrs(pcm_ptrs), _ints(num_samples, n), _ptrs(out_ptrs, n), _ptr(power0),
                  stream=stream)

    def pcm16_to_float_batch(self, C, pcm_ptrs, num_samples, out_ptrs, power0=None, stream=None):
        """One launch for a batch of interleaved int16 payloads (device addresses)."""
        self._pcm16_batch("setk_pcm16_to_float_batch", C, pcm_ptrs, num_samples, out_ptrs, power0, stream)

    def pcm16_channel_stride(self, num_samples):
        return int(self._lib.setk_pcm16_channel_stride(int(num_samples)))

    def pcm16_deinterleave_batch(self, C, pcm_ptrs, num_samples, out_ptrs, power0=None, stream=None):
        """Interleaved int16 frames -> planar int16 [C][pcm16_channel_stride(N)] (device
        addresses), ONE launch: the input layout of FLAG_IN_PCM16."""
        self._pcm16_batch("setk_pcm16_deinterleave_batch", C, pcm_ptrs, num_samples, out_ptrs, power0, stream)

    def kaldi_cm_decode_batch(self, items, stream=None):
        """Kaldi CompressedMatrix bodies -> float32 matrices on the device, ONE launch.  items:
        (kind 'CM' | 'CM2' | 'CM3', vmin, vrange, rows, cols, transpose, src address, dst address);
        the bytes at src are what follows the archive's 16-byte global header (libs/kaldi_io.py
        `uncompress`: same float32 operations, same results bit for bit)."""
        n = len(items)
        col = list(zip(*items)) if n else [()] * 8
        self._run("setk_kaldi_cm_decode_batch", n, _ints([KALDI_KINDS[k] for k in col[0]]),
                  (c_float * n)(*[float(v) for v in col[1]]), (c_float * n)(*[float(v) for v in col[2]]),
                  _ints(col[3]), _ints(col[4]), _ints([bool(v) for v in col[5]]),
                  _ptrs([int(v) for v in col[6]]), _ptrs([int(v) for v in col[7]]), stream=stream)

    def float_to_pcm16(self, audio, C, N, pcm, stream=None):
        """float32 audio[C][N] -> interleaved int16 frames pcm[N][C] (rint(x * 32767), wrapping)."""
        self._run("setk_float_to_pcm16", _ptr(audio), C, N, _ptr(pcm), stream=stream)

    def ban(self, weight, Rn, F, C, out, stream=None):
        self._run("setk_ban", _ptr(weight), _ptr(Rn), F, C, _ptr(out), stream=stream)

    def rank1(self, Rs, Rn, F, C, out, status, stream=None):
        self._run("setk_rank1", _ptr(Rs), _ptr(Rn), F, C, _ptr(out), _ptr(status), stream=stream)

    def beamform(self, weight, spec, C, T, F, out, stream=None):
        self._run("setk_beamform", _ptr(weight), _ptr(spec), C, T, F, _ptr(out), stream=stream)

    # -- CGMM and CACGMM mask estimation ----------------------------------------
    def cgmm_masks(self, spec, C, T, F, num_iters, init_mask, gamma_out, mask_out, stream=None,
                   update_alpha=False):
        self._run("setk_cgmm_masks", _ptr(spec), C, T, F, int(num_iters), _ptr(init_mask), _ptr(gamma_out),
                  _ptr(mask_out), CGMM_UPDATE_ALPHA if update_alpha else 0, stream=stream)

    def cgmm_masks_k(self, spec, C, T, F, K, num_iters, gamma0, init_mask, gamma_out, stream=None,
                     update_alpha=False, status=None):
        """General CGMM (K <= 4 classes, C <= 16 channels): spec [C][T][F] complex64, gamma0
        [K][F][T] float64 or None (K = 2: init_mask [T][F] or the deterministic start),
        gamma_out [K][T][F] float32; status int32[F] (numpy or device address) or None: SETK_NUM_*
        per bin (non-finite covariance, Jacobi sweep limit -- numpy.linalg.eigh's LinAlgError)."""
        self._run("setk_cgmm_masks_k_status", _ptr(spec), int(C), int(T), int(F), int(K), int(num_iters),
                  _ptr(gamma0), _ptr(init_mask), _ptr(gamma_out), CGMM_UPDATE_ALPHA if update_alpha else 0,
                  _ptr(status), stream=stream)

    def cgmm_masks_batch(self, C, spec_ptrs, num_frames, F, num_iters, init_ptrs, out_ptrs,
                         stream=None, update_alpha=False, spec_pitch=0):
        n = len(spec_ptrs)
        self._run("setk_cgmm_masks_batch", n, int(C), _ptrs(spec_ptrs), _ints(num_frames, n), int(F),
                  int(num_iters), _ptrs(init_ptrs, n), _ptrs(out_ptrs, n),
                  CGMM_UPDATE_ALPHA if update_alpha else 0, int(spec_pitch), stream=stream)

    def cgmm_estimate_batch(self, C, audio_ptrs, num_samples, num_iters, init_ptrs, out_ptrs,
                            stream=None, update_alpha=False):
        """audio in, masks out: STFT straight into the bin-major layout + bin-resident EM.
        Raises SetkUnsupported when a bin of the longest utterance does not fit a CU."""
        n = len(audio_ptrs)
        self._run("setk_cgmm_estimate_batch", n, int(C), _ptrs(audio_ptrs), _ints(num_samples, n),
                  int(num_iters), _ptrs(init_ptrs, n), _ptrs(out_ptrs, n),
                  CGMM_UPDATE_ALPHA if update_alpha else 0, stream=stream)

    def cacgmm_masks(self, spec, C, T, F, K, num_iters, gamma0, gamma_out, stream=None,
                     update_alpha=True, cgmm_init=False, status=None):
        """CACGMM EM (cluster.py:468-535): spec [C][T][F] complex64, gamma0 [K][F][T] float64 (None
        with cgmm_init, K = 2), gamma_out [K][T][F] float32; status int32[F] (numpy or device
        address) or None: SETK_NUM_* per bin (numpy.linalg.eigh's LinAlgError)."""
        self._run("setk_cacgmm_masks", _ptr(spec), int(C), int(T), int(F), int(K), int(num_iters), _ptr(gamma0),
                  cacgmm_flags(update_alpha, cgmm_init), _ptr(gamma_out), _ptr(status), stream=stream)

    def cacgmm_estimate_batch(self, C, audio_ptrs, num_samples, K, num_iters, gamma0_ptrs, out_ptrs,
                              stream=None, update_alpha=True, cgmm_init=False, status=None):
        """audio in, K x T x F masks out: one STFT launch into the bin-major layout, one EM launch.
        gamma0_ptrs: device addresses of the starts [K][257][T] float64 (None with cgmm_init);
        status: int32[n] numpy array or None (worst bin of every utterance)."""
        n = len(audio_ptrs)
        st = _ints((), n) if status is not None else None
        self._run("setk_cacgmm_estimate_batch", n, int(C), _ptrs(audio_ptrs), _ints(num_samples, n), int(K),
                  int(num_iters), _ptrs(gamma0_ptrs, n), cacgmm_flags(update_alpha, cgmm_init),
                  _ptrs(out_ptrs, n), st, stream=stream)
        if status is not None:
            status[:] = list(st)

    # -- directional features, fixed beamformer, WPE, AuxIVA ----------------------
    def directional_feats(self, spec, sv, pairs, C, T, F, out, stream=None):
        """spec [C][T][F], sv [F][C] complex64, pairs [(i, j), ...] -> out [T][F] float32."""
        flat = _ints([v for p in pairs for v in p])
        self._run("setk_directional_feats", _ptr(spec), _ptr(sv), flat, len(flat) // 2, C, T, F, _ptr(out),
                  stream=stream)

    def apply_weights_batch(self, num_channels, audio_ptrs, num_samples, weights, n_sets,
                            weight_index, wave_ptrs, flags=0, stream=None):
        """Fixed beamformer + iSTFT + renorm for a batch; weights [n_sets][257][C]
        complex64 (numpy or device tensor), weight_index: list of ints or None."""
        n = len(audio_ptrs)
        self._run("setk_apply_weights_batch", n, int(num_channels), _ptrs(audio_ptrs), _ints(num_samples, n),
                  _ptr(weights), int(n_sets), _ints(weight_index, n), _ptrs(wave_ptrs, n), int(flags),
                  stream=stream)

    def wpe(self, spec, C, T, F, taps, delay, context, num_iters, out, lambda_enh=None,
            inv_lambda_out=None, status=None, stream=None):
        """spec / out [C][T][F] complex64; status int32[F] (numpy) or None."""
        self._run("setk_wpe", _ptr(spec), int(C), int(T), int(F), int(taps), int(delay), int(context),
                  int(num_iters), _ptr(lambda_enh), _ptr(out), _ptr(inv_lambda_out), _ptr(status), stream=stream)

    def wpe_step(self, spec, C, T, F, taps, delay, lambda_ft, out, status=None, stream=None):
        """One wpe_step with the caller's variances (float64 F x T) used as given."""
        self._run("setk_wpe_step", _ptr(spec), int(C), int(T), int(F), int(taps), int(delay), _ptr(lambda_ft),
                  _ptr(out), _ptr(status), stream=stream)

    def _wpe_batch(self, name, specs, C, frames, F, taps, delay, context, num_iters, outs, status, stream):
        n = len(specs)
        self._run(name, n, _ptrs(specs), int(C), _ints(frames, n), int(F), int(taps), int(delay), int(context),
                  int(num_iters), _ptrs(outs, n), _ptr(status), stream=stream)

    def wpe_batch(self, specs, C, frames, F, taps, delay, context, num_iters, outs, status=None,
                  stream=None):
        """specs / outs: lists of [C][T_u][F] complex64 arrays (numpy or device tensors);
        status int32 [n][F] (numpy) or None."""
        self._wpe_batch("setk_wpe_batch", specs, C, frames, F, taps, delay, context, num_iters, outs, status,
                        stream)

    def wpe_batch_var(self, specs, C, frames, F, taps, delay, context, num_iters, outs, lambda_enh=None,
                      inv_lambda_outs=None, status=None, stream=None):
        """wpe_batch with facted_wpd's per-utterance operands: lambda_enh[u] ([T_u][F] complex64 or
        None) gives the variances of iteration 0, inv_lambda_outs[u] ([T_u][F] float32) receives
        1 / lambda of the last one.  Arrays or device addresses; status int32 [n][F] or None."""
        n = len(specs)
        self._run("setk_wpe_batch_var", n, _ptrs(specs), int(C), _ints(frames, n), int(F), int(taps), int(delay),
                  int(context), int(num_iters), _ptrs(lambda_enh, n), _ptrs(outs, n), _ptrs(inv_lambda_outs, n),
                  _ptr(status), stream=stream)

    def wpe_batch_fnt(self, specs, C, frames, F, taps, delay, context, num_iters, outs, status=None,
                      stream=None):
        """wpe_batch with specs / outs in the reference's layout F x N x T_u (complex64)."""
        self._wpe_batch("setk_wpe_batch_fnt", specs, C, frames, F, taps, delay, context, num_iters, outs,
                        status, stream)

    def auxiva(self, spec, C, T, F, num_epochs, out, status=None, stream=None):
        """auxiva() of apply_auxiva.py:24-57: spec / out [C][T][F] complex64 (numpy or device
        tensors); status int32[F] (numpy or device address) or None: SETK_NUM_* per bin."""
        self._run("setk_auxiva", _ptr(spec), int(C), int(T), int(F), int(num_epochs), _ptr(out), _ptr(status),
                  stream=stream)

    def auxiva_batch(self, C, audio_ptrs, num_samples, num_epochs, wave_ptrs, status=None, flags=0,
                     stream=None):
        """Audio in, separated waves out (device addresses): wave[u] is [C][L_u] float32, or
        int16 with FLAG_OUT_PCM16; status int32[n] (numpy or device address) or None: the worst
        bin of every utterance."""
        n = len(audio_ptrs)
        self._run("setk_auxiva_batch", n, int(C), _ptrs(audio_ptrs), _ints(num_samples, n), int(num_epochs),
                  _ptrs(wave_ptrs, n), _ptr(status), int(flags), stream=stream)

    # -- sound source localisation ------------------------------------------------
    def ssl_scores(self, opts, spec, mask, sv, A, C, T, F, windows, score, index, status=None, stream=None):
        """get_doa of do_ssl.py:30-37 per window: spec [C][T][F] complex64, mask [T][F] float32 or
        None, sv [A][C][F] complex64 (numpy or device tensors); windows a list of (t0, t1) or None
        (the whole utterance); score float64 [W][A] or None, index int32 [W], status int32[1] or
        None (numpy or device addresses)."""
        W = _ints([v for w in windows for v in w]) if windows is not None else None
        self._run("setk_ssl_scores", ctypes.byref(opts), _ptr(spec), _ptr(mask), _ptr(sv), int(A), int(C), int(T),
                  int(F), W, len(windows) if windows is not None else 1, _ptr(score), _ptr(index), _ptr(status),
                  stream=stream)

    def ssl_batch(self, opts, C, audio_ptrs, num_samples, mask_ptrs, sv, A, windows, index, score=None,
                  status=None, stream=None):
        """Audio in, one direction index per window out: audio / mask device addresses (mask_ptrs
        None or a list with None entries), windows a list (per utterance) of lists of (t0, t1);
        index int32 [sum W], score float64 [sum W][A] or None, status int32 [n] or None."""
        n = len(audio_ptrs)
        self._run("setk_ssl_batch", ctypes.byref(opts), n, int(C), _ptrs(audio_ptrs), _ints(num_samples, n),
                  _ptrs(mask_ptrs, n), _ptr(sv), int(A), _ints([v for ws in windows for w in ws for v in w]),
                  _ints([len(ws) for ws in windows], n), _ptr(index), _ptr(score), _ptr(status), stream=stream)

    # -- geometry-driven spatial features -----------------------------------------
    def spatial_feats(self, opts, spec, C, T, F, out, stream=None):
        """One spectrogram spec [C][T][F] complex64 -> out [T][spatial_width(opts, F)] float32 (numpy
        arrays, device tensors or device addresses)."""
        self._run("setk_spatial_feats", ctypes.byref(opts), _ptr(spec), int(C), int(T), int(F), _ptr(out),
                  stream=stream)

    def spatial_batch(self, opts, C, spec_ptrs, num_frames, F, out_ptrs, stream=None):
        """A batch of device spectrograms [C][T_u][F] -> device feature maps, one set of launches."""
        n = len(spec_ptrs)
        self._run("setk_spatial_batch", ctypes.byref(opts), n, int(C), _ptrs(spec_ptrs), _ints(num_frames, n),
                  int(F), _ptrs(out_ptrs, n), stream=stream)

    # -- OM-LSA noise suppression ---------------------------------------------------
    def ns_gain(self, opts, spec, T, F, gain=None, out=None, status=None, stream=None):
        """MCRA.run / iMCRA.run of libs/ns.py on one spectrogram spec [T][F] complex64: gain [T][F]
        float64 and / or out [T][F] complex64 = gain x spec as opts.flags select (numpy arrays,
        device tensors or device addresses); status int32[1] or None."""
        self._run("setk_ns_gain", ctypes.byref(opts), _ptr(spec), int(T), int(F), _ptr(gain), _ptr(out),
                  _ptr(status), stream=stream)

    def ns_batch(self, opts, audio_ptrs, num_samples, wave_ptrs=None, gain_ptrs=None, status=None, flags=0,
                 stream=None):
        """Single-channel audio in (device addresses; int16 with FLAG_IN_PCM16), waveforms (float32,
        or int16 with FLAG_OUT_PCM16) and / or gains float64 [T_u][257] out as opts.flags select;
        status int32[n] (numpy or device address) or None."""
        n = len(audio_ptrs)
        self._run("setk_ns_batch", ctypes.byref(opts), n, _ptrs(audio_ptrs), _ints(num_samples, n),
                  _ptrs(wave_ptrs, n), _ptrs(gain_ptrs, n), _ptr(status), int(flags), stream=stream)

    def expint_e1(self, x, y, stream=None):
        """y = E1(x), float64 (numpy arrays or device tensors of the same size)."""
        n = x.size if isinstance(x, np.ndarray) else x.numel()
        self._run("setk_expint_e1", _ptr(x), _ptr(y), int(n), stream=stream)

    # -- oracle TF masks and mask-based separation -----------------------------------
    @staticmethod
    def _stats_out(stats):
        """[(over, below, below_sum), ...] of a TfmaskStats array."""
        return [(int(s.over), int(s.below), float(s.below_sum)) for s in stats]

    def tf_mask(self, kind, tgt, mix, T, F, mask, cutoff=-1.0, want_stats=True, stream=None):
        """compute_mask.py's compute_mask and clips on stored spectra tgt, mix [T][F] complex64: mask
        [T][F] float32 ([T][2F] for crm); numpy arrays, device tensors or device addresses.  Returns
        (cells over the cutoff, cells below zero, their sum) or None."""
        st = (TfmaskStats * 1)() if want_stats else None
        self._run("setk_tf_mask", tfmask_kind(kind), _ptr(tgt), _ptr(mix), int(T), int(F), float(cutoff), _ptr(mask),
                  ctypes.addressof(st) if want_stats else None, stream=stream)
        return self._stats_out(st)[0] if want_stats else None

    def tf_apply(self, spec, mask, T, F, out, phase_ref=None, stream=None):
        """out = spec x mask, or |spec| x mask x exp(i angle(phase_ref)); [T][F] each."""
        self._run("setk_tf_apply", _ptr(spec), _ptr(mask), _ptr(phase_ref), int(T), int(F), _ptr(out), stream=stream)

    def tf_mask_batch(self, kind, tgt_ptrs, mix_ptrs, num_samples, mask_ptrs, cutoff=-1.0, status=None, flags=0,
                      want_stats=True, stream=None):
        """Pairs of device waveforms (int16 with FLAG_IN_PCM16) -> device masks float32 [T_u][257]
        ([T_u][514] for crm) in one fused launch; status int32[n] or None.  Returns the statistics of
        every utterance or None."""
        n = len(mix_ptrs)
        st = (TfmaskStats * n)() if want_stats else None
        self._run("setk_tf_mask_batch", tfmask_kind(kind), n, _ptrs(tgt_ptrs, n), _ptrs(mix_ptrs), _ints(num_samples, n),
                  float(cutoff), _ptrs(mask_ptrs, n), ctypes.addressof(st) if want_stats else None, _ptr(status),
                  int(flags), stream=stream)
        return self._stats_out(st) if want_stats else None

    def tf_separate_batch(self, mix_ptrs, num_samples, mask_ptrs, wave_ptrs, phase_ptrs=None, norm=None, nsamps=None,
                          status=None, flags=0, stream=None):
        """Device mixtures and device masks [T_u][257] -> device waveforms: one fused forward launch,
        one inverse launch, one scaling launch.  norm: per utterance, > 0 renorms to that max-abs;
        nsamps: per utterance, >= 0 keeps that length."""
        n = len(mix_ptrs)
        norm = None if norm is None else np.ascontiguousarray(norm, dtype=np.float32)
        self._run("setk_tf_separate_batch", n, _ptrs(mix_ptrs), _ptrs(phase_ptrs, n), _ints(num_samples, n),
                  _ptrs(mask_ptrs, n), _ptr(norm), _ints(nsamps, n), _ptrs(wave_ptrs, n), _ptr(status), int(flags),
                  stream=stream)

    def oracle_separate_batch(self, kind, num_targets, mix_ptrs, target_ptrs, num_samples, wave_ptrs, nsamps=None,
                              status=None, flags=0, stream=None):
        """Device mixtures and num_targets device references each (target_ptrs[u * K + k]) -> device
        waveforms wave_ptrs[u * K + k] = inverse_stft(mixture x mask_k)."""
        n = len(mix_ptrs)
        self._run("setk_oracle_separate_batch", tfmask_kind(kind), n, int(num_targets), _ptrs(mix_ptrs),
                  _ptrs(target_ptrs), _ints(num_samples, n), _ints(nsamps, n), _ptrs(wave_ptrs), _ptr(status),
                  int(flags), stream=stream)

    # -- SI-SNR scoring ---------------------------------------------------------------
    def si_snr_batch(self, num_src, est_ptrs, est_strides, ref_ptrs, ref_strides, num_samples, pair, best=None,
                     perm=None, status=None, eps=1e-8, flags=0, stream=None):
        """si_snr of every (estimate, reference) pair of every utterance and permute_si_snr over
        them (libs/metric.py:13-60).  num_src: K_u per utterance; est_ptrs / ref_ptrs: sum(K_u)
        device addresses, utterance-major, with their sample strides; pair float64 [sum K_u^2],
        best float64 [n], perm int32 [sum K_u], status int32 [n] (numpy arrays or device
        addresses; all but pair may be None).  flags: FLAG_IN_PCM16 | FLAG_KEEP_DC."""
        n, m = len(num_src), len(est_ptrs)
        self._run("setk_si_snr_batch", n, _ints(num_src), _ptrs(est_ptrs), _ints(est_strides, m), _ptrs(ref_ptrs, m),
                  _ints(ref_strides, m), _ints(num_samples, n), float(eps), int(flags), _ptr(pair), _ptr(best),
                  _ptr(perm), _ptr(status), stream=stream)

    def si_snr(self, x, s, eps=1e-8, flags=0, stream=None):
        """si_snr of one pair of float32 vectors (int16 with FLAG_IN_PCM16; numpy arrays or device
        tensors of one size): a Python float."""
        n = x.size if isinstance(x, np.ndarray) else x.numel()
        out = np.empty(1, dtype=np.float64)
        self._run("setk_si_snr", _ptr(x), _ptr(s), int(n), float(eps), int(flags), _ptr(out), stream=stream)
        return float(out[0])

    # -- data simulation ------------------------------------------------------------
    def fir_reverb(self, spk, S, rir, N, R, out, power0=None, flags=0, stream=None):
        """add_room_response: spk [S] float32 (int16 with FLAG_IN_PCM16), rir [N][R] float32 -> out
        [N][S] float32 and, when asked, power0 float64[1] = mean(out[0]**2) (numpy arrays, device
        tensors or device addresses)."""
        self._run("setk_fir_reverb", _ptr(spk), int(S), _ptr(rir), int(N), int(R), _ptr(out), _ptr(power0),
                  int(flags), stream=stream)

    def simu_batch(self, recipes, status=None, flags=0, stream=None):
        """run_simu for a list of simu_recipe structures (device buffers in and out); status int32[n]
        (numpy or device address) or None."""
        n = len(recipes)
        self._run("setk_simu_batch", n, (SimuRecipe * n)(*recipes), _ptr(status), int(flags), stream=stream)

    # -- room impulse responses -----------------------------------------------------
    def rir_generate_batch(self, specs, outs, status=None, flags=0, stream=None):
        """GenerateRir for a list of rir_spec structures; outs[r] float32 [n_mics][num_samples] (numpy
        arrays or device addresses), status int32[n] (numpy or device address) or None."""
        n = len(specs)
        self._run("setk_rir_generate_batch", n, (RirSpec * n)(*specs), _ptrs(outs, n), _ptr(status), int(flags),
                  stream=stream)

    def rir_generate(self, spec, out=None, flags=0, stream=None):
        """One RIR: (float32 [n_mics][num_samples], its SETK_NUM_* status)."""
        if out is None:
            out = np.empty((spec.n_mics, spec.num_samples), dtype=np.float32)
        status = np.zeros(1, dtype=np.int32)
        self._run("setk_rir_generate", ctypes.byref(spec), _ptr(out), _ptr(status), int(flags), stream=stream)
        return out, int(status[0])

    # -- fused hot path ---------------------------------------------------------
    def enhance_batch(self, opts, num_channels, audio_ptrs, num_samples, mask_ptrs,
                      itf_ptrs, wave_ptrs, want_status=True, stream=None, taps=None,
                      status_ptr=None):
        """taps: dict with any of Rs, Rn ([n][F][C][C] complex64), weight ([n][F][C]
        complex64), maxabs ([n] float32) -> numpy arrays / device tensors filled by
        setk_enhance_batch_taps."""
        n = len(audio_ptrs)
        ST = _ints((), n) if want_status else None
        if status_ptr is not None:
            # device int32[n]: filled asynchronously on the stream, nothing returned
            ST = ctypes.cast(c_void_p(int(status_ptr)), POINTER(c_int))
            want_status = False
        args = (ctypes.byref(opts), n, int(num_channels), _ptrs(audio_ptrs), _ints(num_samples, n),
                _ptrs(mask_ptrs, n), _ptrs(itf_ptrs, n), _ptrs(wave_ptrs, n), ST)
        if taps:
            tp = BatchTaps(*[_ptr(taps.get(k)) for k in ("Rs", "Rn", "weight", "maxabs")])
            self._run("setk_enhance_batch_taps", *args, ctypes.byref(tp), stream=stream)
        else:
            self._run("setk_enhance_batch", *args, stream=stream)
        return list(ST) if want_status else None

    # -- block-online beamforming -------------------------------------------------
    def online_num_chunks(self, num_samples, chunk_size):
        """ceil(T / chunk_size) under the plan: the chunks of one utterance."""
        n = self._lib.setk_online_num_chunks(self._h, int(num_samples), int(chunk_size))
        if n < 0:
            self.check(n)
        return n

    def enhance_online_batch(self, opts, chunk_size, alpha, num_channels, audio_ptrs, num_samples, mask_ptrs,
                             itf_ptrs, wave_ptrs, status=None, taps=None, stream=None):
        """setk_enhance_online_batch.  status: int32[n] (numpy or a device address) or None; taps:
        dict with any of Rs, Rn ([chunks_total][F][C][C] complex64) and weight ([chunks_total][F][C]
        complex64), numpy arrays or device addresses."""
        n = len(audio_ptrs)
        online = OnlineOpts(int(chunk_size), float(alpha))
        tp = OnlineTaps(*[_ptr(taps.get(k)) for k in ("Rs", "Rn", "weight")]) if taps else None
        st = None if status is None else ctypes.cast(c_void_p(_ptr(status)), POINTER(c_int))
        self._run("setk_enhance_online_batch", ctypes.byref(opts), ctypes.byref(online), n, int(num_channels),
                  _ptrs(audio_ptrs), _ints(num_samples, n), _ptrs(mask_ptrs, n), _ptrs(itf_ptrs, n),
                  _ptrs(wave_ptrs, n), st, ctypes.byref(tp) if tp else None, stream=stream)

    # -- stage timings ------------------------------------------------------------
    def set_profiling(self, on):
        self.check(self._lib.setk_set_profiling(self._h, 1 if on else 0))

    def last_stage_ms(self):
        out = (c_float * 4)()
        self.check(self._lib.setk_last_stage_ms(self._h, out))
        return list(out)


_default_ctx = {}


def default_context(device=None):
    """Process-wide context for the python API mirror (one per device)."""
    if device is None:
        # SETK_DEVICE, then LOCAL_RANK (torchrun), then torch's current device
        if os.environ.get("SETK_DEVICE") is not None:
            device = int(os.environ["SETK_DEVICE"])
        elif os.environ.get("LOCAL_RANK") is not None:
            device = int(os.environ["LOCAL_RANK"])
        else:
            device = 0
            torch = _torch()
            try:
                if torch is not None and torch.cuda.is_available():
                    device = torch.cuda.current_device()
            except Exception:
                pass
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
