"""The operand split's arithmetic contract (csrc/operand_split.h) on the CPU: the header's splits and scales
are __host__ __device__, so a stand-alone program (tests/operand_split_host.hip, host pass only) runs them over seeded values
and prints what it found; the bounds below follow from the number formats.  What the kernels do with the pieces on the GPU
is held per element by tests/test_gpu_operand_scheme.py."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def found(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("operand_split") / "operand_split_host")
    subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "operand_split_host.hip"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    print(out)
    return {k: float(v) for k, v in (line.split() for line in out.splitlines())}


def test_three_bf16_pieces_are_exact(found):
    # 10^6 pairs, exponents -27 .. +22, both signs: low halves -> first argument, high halves -> second, bit for bit
    assert found["np3_values"] == 1000000
    assert found["np3_bad_lo"] == 0 and found["np3_bad_hi"] == 0


def test_two_fp16_pieces_keep_22_bits_near_the_block_maximum(found):
    # |v| in [2^-2, 2^15): within 2^16 of a block maximum in [2^14, 2^15); both halves of every pair
    assert found["np2_rel_values"] == 4000000
    assert found["np2_rel_worst_log2"] <= -22.0


def test_two_fp16_pieces_bound_the_absolute_error_below(found):
    # |v| in [2^-40, 2^-2): half a unit of fp16's denormal grid
    assert found["np2_abs_values"] == 1000000
    assert found["np2_abs_worst_log2"] <= -25.0


@pytest.mark.parametrize("name", ["block_scale", "weight_scale"])
def test_scales_over_every_exponent(found, name):
    # every biased exponent 0 .. 255 (zero, denormals, infinity, NaN included): inside 16 .. 250 the maximum lands in its
    # window and S * (1 / S) == 1 exactly, outside both factors are exactly 1
    assert found[name + "_checked"] == 256 * 4
    assert found[name + "_bad"] == 0


def test_quad_split_is_two_pair_splits(found):
    assert found["quad3_bad"] == 0 and found["quad2_bad"] == 0
