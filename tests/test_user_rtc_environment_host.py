"""The run-time compiler of user models and costs (csrc/user_rtc.hip) lives in a link namespace of its own, whose C library keeps
its own environment pointer.  A process that changes os.environ between two compiles -- the suite does, with monkeypatch.setenv --
moves the environment array; the second compile must read the current one.  No GPU needed: the compile is host work."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import ctypes, os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "tests"), os.path.join(sys.argv[1], "ilqr-admm_amd"), sys.argv[1]]
import reg_reference as R
from isls import _capi as capi
os.environ["ISLS_TEST_BEFORE"] = "1"                     # from here on the environment array is a heap block
first = capi.user_cost_create(R.BumpCost.SOURCE, 4, 2, 5)
n0 = len(os.environ)
for i in range(300):                                     # the array grows: it moves, and its old block is freed
    os.environ[f"ISLS_TEST_VAR_{i}"] = "x"
libc = ctypes.CDLL(None)
libc.malloc.restype = ctypes.c_void_p
for size in range((n0 - 4) * 8, (n0 + 12) * 8, 8):       # blocks of the old array's size, filled with what is no pointer
    for _ in range(64):
        ctypes.memset(libc.malloc(size), 0x41, size)
second = capi.user_cost_create(R.BumpCost.SOURCE + "\n", 4, 2, 5)
print("compiled", first, second)
'''


def test_compile_after_the_environment_has_moved():
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stdout.split()[0] == "compiled" and int(r.stdout.split()[2]) == int(r.stdout.split()[1]) + 1
