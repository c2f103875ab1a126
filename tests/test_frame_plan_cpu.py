"""The input-layout table and the frame plan (jpgenc_amd/csrc/layouts.hpp, frame_plan.cpp), without a GPU:

- every layout's row against a statement written out by hand, and the codes that are no layout;
- every refusal of plan_frame beside its nearest accepted frame, with its error code;
- the upload of a host frame, simulated: the plan's copies executed with memcpy, and every sample
  read back at the address the device pitches give it;
- the coded size under every orientation and downscale factor.

All of it is a stand-alone host program (tests/cpp/test_frame_plan.cpp), run plain and under
AddressSanitizer + UBSan.  Nothing is loaded into Python.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("table_valid_codes", "table_rows", "table_capabilities", "refuse_null_pointer", "refuse_maxval_0",
          "refuse_maxval_0_null_pointer", "refuse_device_frame_at_offset_bound", "stripe_settings", "upload_layout_0",
          "upload_layout_17", "upload_layout_42", "upload_layout_48", "coded_size")


def _check(rc, out):
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert rc == 0 and out.rstrip().endswith("all ok") and "FAIL" not in out, out[-4000:]


@pytest.fixture(scope="module")
def plain():
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "test_frame_plan")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout + r.stderr


def test_frame_plan(plain):
    _check(*plain)


@pytest.mark.parametrize("group", GROUPS)
def test_frame_plan_ran(plain, group):
    assert f"ok {group}" in plain[1].splitlines(), plain[1][-2000:]


def test_frame_plan_sanitized():
    # built as the other sanitized host programs are (make asan's flags), this one target only
    exe = os.path.join("tests", "cpp", "bin", "asan", "test_frame_plan")
    r = subprocess.run(["make", "-s", exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, exe)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    _check(r.returncode, r.stdout + r.stderr)
