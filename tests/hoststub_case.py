"""What the tests on the plain HIP stand-in (tools/hoststub, PLAIN=1) share: the parent side builds
the stand-in and runs the test file as a child process whose SETK_LIB names it (SETK_LIB is read at
import), the child side reads the stand-in's counters."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_child(test_file, ok_line, *args):
    """Build the stand-in, run `test_file` (its `_child`) on it and expect `ok_line` in its output."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "hoststub", "build.sh")], capture_output=True,
                       text=True, timeout=900, env=dict(os.environ, PLAIN="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, SETK_ALLOW_HOSTSTUB="1", SETK_TORCH_FREE="1", OMP_NUM_THREADS="1",
               SETK_LIB=os.path.join(ROOT, "_abl", "libsetk_hoststub.so"),
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("HOSTSTUB_TRACE", None)
    r = subprocess.run([sys.executable, os.path.abspath(test_file), *args], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert ok_line in r.stdout, r.stdout[-2000:]


def report():
    """hoststub_report: [launches, violations, copies, live allocations, the first violation]."""
    from setk_amd import _ffi
    vals = [ctypes.c_long() for _ in range(4)]
    first = ctypes.create_string_buffer(512)
    _ffi.load_library().hoststub_report(*[ctypes.byref(v) for v in vals], first, 512)
    return [v.value for v in vals] + [first.value.decode()]
