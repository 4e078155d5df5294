"""The host side of setk_auxiva / setk_auxiva_batch under AddressSanitizer + UBSan, no GPU: the
recipe of tests/test_host_asan.py (library rebuilt host-only against tools/hoststub/hip_stub.cpp,
whose launches validate their geometry and whose copies bound-check the device side) with
tests/host_asan_auxiva_driver.py as the caller."""
import os
import subprocess
import sys

import pytest

from test_host_asan import ROOT, _runtime


@pytest.fixture(scope="module")
def asan_env():
    rt = _runtime()
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "hoststub", "build.sh")], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ)
    env.update(LD_PRELOAD=rt, SETK_LIB=os.path.join(ROOT, "_abl", "libsetk_hostasan.so"),
               SETK_PIN_CAP_KB="64", SETK_ALLOW_HOSTSTUB="1", SETK_TORCH_FREE="1",
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return env


def test_auxiva_entry_points_are_clean_under_the_sanitizers(asan_env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_asan_auxiva_driver.py")],
                       capture_output=True, text=True, env=asan_env, timeout=900)
    assert r.returncode == 0 and "ASAN_DRIVE_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    assert "channels <= 8" in r.stdout
