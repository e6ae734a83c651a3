"""Memory contract of the stride-4 transposed-conv routes (ConvTranspose1d k = 8, stride 4, padding 2), through ctypes on
tests/memcheck.py's guarded arena with tests/test_gpu_memcontract.py's convt_case: guard bands around every buffer, the
exact queried workspace, outputs and workspace poisoned twice (NaN pattern, 1e30) with bitwise-equal results, inputs
unchanged, values against the CPU oracle -- for the three passes on their matrix-pipe kernels at a small shape each, and
for the calls a route declines (an operand or the workspace 4 bytes past a 16-byte boundary): they still succeed, on the
kernel behind, with the guards intact."""
import pytest

from test_gpu_memcontract import Case, convt_case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = []


def case(id, fn, *args):
    CASES.append(Case(id, (), fn, args))


# name, B, Cin, L, Cout, K, stride, pad
SMALL = ("mc_ct_s4_small", 2, 32, 16, 8, 8, 4, 2)          # too few output channels for the forward's row tiles
ROWS = ("mc_ct_s4_rows", 32, 128, 32, 64, 8, 4, 2)         # one 64-sample chunk rows: three-tap forward, two-tap backward
PAIRED = ("mc_ct_s4_paired", 8, 64, 1028, 64, 8, 4, 2)     # >= 128 workgroups: the paired split-bf16 forward, a tile tail
TWO_TAP = ("mc_ct_s4_two_tap", 16, 40, 1028, 32, 8, 4, 2)   # 40 channels: chunks of 8 only, the fp32 two-tap kernel, a tile tail

# the routes on their kernels, exact workspace
case("s4_TF_MFMA_rows2", convt_case, ROWS, 0, "k_conv_rows2")
case("s4_TF_MFMA_rows3p", convt_case, PAIRED, 0, "k_conv_rows3p")
case("s4_TF_MFMA_rows2_two_tap", convt_case, TWO_TAP, 0, "k_conv_rows2")
case("s4_TF_DIRECT_small", convt_case, SMALL, 0, "k_conv1d_bwd_data_direct")
case("s4_TD_MFMA_small", convt_case, SMALL, 1, "k_conv_rows2")
case("s4_TD_MFMA_rows2", convt_case, ROWS, 1, "k_conv_rows2")
case("s4_TW_MFMA_wrows", convt_case, ROWS, 2, "k_wgrad_rows")
case("s4_TW_MFMA_igemm_small", convt_case, SMALL, 2, "k_igemm_wgrad")

# declines.  Forward: the phase-interleaving epilogues store 16 bytes, an output at a 4-byte address goes to the direct kernel;
# x at a 4-byte address leaves the pipelined kernels for the first-generation row kernel (dword loads).
case("s4_TF_MFMA_declines_y_plus4", convt_case, ROWS, 0, "k_conv1d_bwd_data_direct", {"y": 4}, "exact", "k_conv_rows2")
case("s4_TF_MFMA_rows3p_declines_y_plus4", convt_case, PAIRED, 0, "k_conv1d_bwd_data_direct", {"y": 4}, "exact", "k_conv_rows3p")
case("s4_TF_MFMA_x_plus4", convt_case, ROWS, 0, "k_conv_mfma_rows", {"x": 4}, "exact", "k_conv_rows2")
# backward data: k_conv_mfma_rows reads the phase-split gradient as dwords; with gx at a 4-byte address these launches stay
# on the pipelined kernel (they are split-K: its slabs go to the workspace, the slab sum writes gx as dwords)
for _op in ("gy", "y_act"):
    case("s4_TD_MFMA_rows_%s_plus4" % _op, convt_case, ROWS, 1, "k_conv_mfma_rows", {_op: 4}, "exact", "k_conv_rows2")
case("s4_TD_MFMA_rows_gx_plus4", convt_case, ROWS, 1, None, {"gx": 4})
# weight gradient: the row-tile kernel loads 16 bytes, the im2col form behind it dwords
for _op in ("x", "gy", "y_act"):
    case("s4_TW_MFMA_declines_%s_plus4" % _op, convt_case, ROWS, 2, "k_igemm_wgrad", {_op: 4}, "exact", "k_wgrad_rows")
# the workspace at a 4-byte address: forward and backward data need the packed weights on the 16-byte grid and pass the call
# on to the direct kernels; the weight gradient's own workspace accesses are dwords
case("s4_TF_MFMA_declines_ws_plus4", convt_case, ROWS, 0, "k_conv1d_bwd_data_direct", None, "plus4", "k_conv_rows2")
case("s4_TD_MFMA_declines_ws_plus4", convt_case, ROWS, 1, "k_conv1d_fwd_direct", None, "plus4", "k_conv_rows2")
case("s4_TW_MFMA_ws_plus4", convt_case, ROWS, 2, None, None, "plus4")
# ... and no workspace at all: the direct kernels need none
case("s4_TF_MFMA_declines_null_ws", convt_case, ROWS, 0, "k_conv1d_bwd_data_direct", None, "null", "k_conv_rows2")
case("s4_TD_MFMA_declines_null_ws", convt_case, ROWS, 1, "k_conv1d_fwd_direct", None, "null", "k_conv_rows2")


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_memory_contract_convt_s4(c):
    c.fn(*c.args)
