"""The AuxIVA entry points of include/setk_hip.h against the host-only sanitizer build (see
tests/host_asan_driver.py, whose recipe this follows): host and device pointers, zero / one /
several epochs, odd F and T, ragged batches with a 30 s utterance, float32 and PCM16 out,
profiling events, the channel bound.

    LD_PRELOAD=<libclang_rt.asan> SETK_ALLOW_HOSTSTUB=1 SETK_LIB=_abl/libsetk_hostasan.so python tests/host_asan_auxiva_driver.py
"""
import ctypes
import os
import sys
from ctypes import byref, c_void_p, c_size_t, c_int
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from setk_amd import _ffi
lib = _ffi.load_library()
assert hasattr(lib, "hoststub_report"), "not the host-stub build: set SETK_LIB"
lib.hipMalloc.argtypes = [ctypes.POINTER(c_void_p), c_size_t]
lib.hipFree.argtypes = [c_void_p]
lib.hipMemcpy.argtypes = [c_void_p, c_void_p, c_size_t, c_int]
rng = np.random.default_rng(0)
def dmalloc(n):
    p = c_void_p(); assert lib.hipMalloc(byref(p), max(int(n), 16)) == 0; return p.value
def to_dev(a):
    a = np.ascontiguousarray(a); p = dmalloc(a.nbytes); assert lib.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0; return p
ctx = _ffi.Context(0)
for C, T, F in ((1, 5, 257), (3, 131, 129), (8, 300, 257)):
    X = (rng.standard_normal((C, T, F)) + 1j * rng.standard_normal((C, T, F))).astype(np.complex64)
    for ep in (0, 1, 3):
        out = np.empty_like(X); st = np.zeros(F, np.int32)
        ctx.auxiva(X, C, T, F, ep, out, status=st)
        ctx.auxiva(to_dev(X), C, T, F, ep, dmalloc(X.nbytes), status=dmalloc(4 * F))
try:
    ctx.auxiva(np.zeros((9, 4, 257), np.complex64), 9, 4, 257, 1, np.zeros((9, 4, 257), np.complex64))
    raise SystemExit("no refusal")
except _ffi.SetkUnsupported as e:
    print("refused:", e)
ctx.stft_plan(512, 256, 512, True)
for C, lens in ((1, (600, 16000)), (5, (480000, 20000, 33333)), (8, (40000,))):
    for pcm in (0, _ffi.FLAG_OUT_PCM16):
        audio = [to_dev(rng.standard_normal((C, N)).astype(np.float32)) for N in lens]
        Ls = [ctx.istft_num_samples(ctx.num_frames(N)) for N in lens]
        waves = [dmalloc(C * L * (2 if pcm else 4)) for L in Ls]
        st = np.zeros(len(lens), np.int32)
        ctx.set_profiling(pcm != 0)
        ctx.auxiva_batch(C, audio, lens, 2, waves, status=st, flags=pcm)
        ctx.auxiva_batch(C, audio, lens, 0, waves, status=dmalloc(4 * len(lens)), flags=pcm)
        if pcm:
            print("stage ms", ctx.last_stage_ms())
print("ASAN_DRIVE_OK")
