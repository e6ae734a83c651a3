"""The memory-contract harness itself (tests/memcheck.py) on CPU tensors: every defect it exists to catch is planted once and
must be reported with the right buffer name -- and the table of tests/test_gpu_memcontract.py must name every C-ABI entry
that touches device memory."""
import pytest

torch = pytest.importorskip("torch")

from memcheck import Arena, MemcheckError, MS_OK, MS_ERR_INVALID_ARG    # noqa: E402


def _setup():
    """y = 2 x with a 100-byte workspace: the buffers of one well-behaved call."""
    a = Arena("cpu", capacity=2 << 20)
    x = a.put(torch.arange(37, dtype=torch.float32), "input", name="x")
    y = a.take((37,), "output", offset_bytes=4, name="y")
    acc = a.put(torch.ones(5), "accumulate", name="acc")
    ws = a.take(100, "workspace", name="ws")
    return a, x, y, acc, ws


def _good(a, x, y, acc, ws):
    def call():
        ws.t.fill_(3)
        y.t.copy_(2 * x.t)
        acc.t.add_(1)
        return MS_OK
    return call


def test_placement():
    a, x, y, acc, ws = _setup()
    assert x.ptr % 256 == 0 and y.ptr % 256 == 4 and ws.ptr % 256 == 0 and ws.t.numel() == 100
    assert y.t.dtype == torch.float32 and y.t.is_contiguous()
    words = a.take((6,), "output", dtype=torch.int32, name="signs")
    assert words.t.dtype == torch.int32
    for b in a.bufs:
        assert b.start - b.lo >= 64 * 1024 and b.hi - (b.start + b.nbytes) == 64 * 1024
        assert b.hi < a.block.numel()                    # never flush against the end of the block
    with pytest.raises(MemcheckError):
        a.take((1 << 20,), "output", name="too_big")


def test_untouched_run_passes():
    a, x, y, acc, ws = _setup()
    rc, out = a.run_twice(_good(a, x, y, acc, ws))
    assert rc == MS_OK and torch.equal(out["y"], 2 * x.t) and torch.equal(out["acc"], torch.full((5,), 2.0))


def _problems_after(mutate):
    a, x, y, acc, ws = _setup()
    a.arm("nan")
    _good(a, x, y, acc, ws)()
    mutate(a, x, y, acc, ws)
    return a.problems()


def test_write_one_past_an_output_is_caught():
    def m(a, x, y, acc, ws):
        a.block[y.start + y.nbytes:y.start + y.nbytes + 4].view(torch.float32).fill_(1.0)
    p = _problems_after(m)
    assert len(p) == 1 and "guard behind output 'y'" in p[0] and "offsets +0 .. +3 from its end" in p[0], p


def test_write_one_before_an_output_is_caught():
    def m(a, x, y, acc, ws):
        a.block[y.start - 4:y.start].view(torch.float32).fill_(1.0)
    p = _problems_after(m)
    assert len(p) == 1 and "guard before output 'y'" in p[0] and "offsets -4 .. -1 from its start" in p[0], p


def test_skipped_output_element_is_caught():
    for poison in ("nan", "big"):
        a, x, y, acc, ws = _setup()
        a.arm(poison)
        _good(a, x, y, acc, ws)()
        a.arm(poison)                                     # (re-poison, then write all but element 11)
        y.t[:11] = 2 * x.t[:11]
        y.t[12:] = 2 * x.t[12:]
        p = a.problems()
        assert len(p) == 1 and "output 'y': 1 of 37 element(s) never written, first at element 11" in p[0], p


def test_changed_input_is_caught():
    def m(a, x, y, acc, ws):
        x.t[3] = -1.0
    p = _problems_after(m)
    assert len(p) == 1 and "input 'x' changed" in p[0] and "1 element(s), first at element 3" in p[0], p


def test_byte_past_the_workspace_is_caught():
    def m(a, x, y, acc, ws):
        a.block[ws.start + 100] = 0
    p = _problems_after(m)
    assert len(p) == 1 and "guard behind workspace 'ws'" in p[0] and "offsets +0 .. +0 from its end" in p[0], p


def test_everything_is_reported_at_once():
    def m(a, x, y, acc, ws):
        x.t[0] = 9.0
        a.block[ws.start + 100] = 0
        a.block[y.start - 1] = 0
    p = _problems_after(m)
    assert len(p) == 3, p
    with pytest.raises(MemcheckError):
        a, x, y, acc, ws = _setup()
        a.arm("nan")
        a.verify()                                        # nothing written at all


def test_run_twice_catches_reads_of_unwritten_scratch():
    a, x, y, acc, ws = _setup()
    scratch = ws.raw[:96].view(torch.float32)

    def stale():                                          # sums a workspace slab it never wrote
        y.t.copy_(2 * x.t)
        y.t[5] += 1.0 if bool(scratch[7] == 1e30) else 0.0
        acc.t.add_(1)
        return MS_OK
    with pytest.raises(MemcheckError, match="'y' depends on prior scratch / output contents.*first at element 5"):
        a.run_twice(stale)

    def unstable_status():
        return MS_OK if a.poison == "nan" else MS_ERR_INVALID_ARG
    with pytest.raises(MemcheckError):
        a.run_twice(unstable_status)


def test_refusing_call_must_write_nothing():
    a, x, y, acc, ws = _setup()
    rc, _ = a.run_twice(lambda: MS_ERR_INVALID_ARG)
    assert rc == MS_ERR_INVALID_ARG

    def refuses_late():
        y.t[0] = 1.0
        return MS_ERR_INVALID_ARG
    with pytest.raises(MemcheckError, match="written by a call that refused"):
        a.run_twice(refuses_late)


def test_partial_output_is_compared_where_written():
    a = Arena("cpu", capacity=1 << 20)
    img = a.take((16,), "output", name="image", partial=True)

    def pack():
        img.t[:10] = torch.arange(10, dtype=torch.float32)
        return MS_OK
    rc, out = a.run_twice(pack)
    assert rc == MS_OK and torch.equal(out["image"][:10], torch.arange(10, dtype=torch.float32))

    def moving():                                         # writes another set of elements the second time
        img.t[:10 if a.poison == "nan" else 11] = 1.0
        return MS_OK
    with pytest.raises(MemcheckError, match="set of written elements"):
        a.run_twice(moving)
    with pytest.raises(MemcheckError, match="nothing written"):
        a.run_twice(lambda: MS_OK)


def test_tolerance_mode_names_the_route():
    a, x, y, acc, ws = _setup()

    def atomics():
        y.t.copy_(2 * x.t)
        y.t[4] *= 1.0 + (1e-7 if a.poison == "nan" else 0.0)
        acc.t.add_(1)
        return MS_OK
    a.run_twice(atomics, tol=("k_reflect_fold_bwd", 1e-4))
    with pytest.raises(MemcheckError, match="k_reflect_fold_bwd"):
        a.run_twice(atomics, tol=("k_reflect_fold_bwd", 1e-9))


# ---------------------------------------------------------------- completeness of the GPU table

# entries without a memory-contract case, each with its reason: host-side queries and the comm / profile / debug aids only
EXEMPT = {
    "ms_version": "host-only: returns a constant",
    "ms_status_string": "host-only: static strings",
    "ms_conv1d_out_len": "host-only geometry query",
    "ms_convt1d_out_len": "host-only geometry query",
    "ms_conv1d_workspace_bytes": "host-only size query (its result is the exact workspace size of the conv cases)",
    "ms_convt1d_workspace_bytes": "host-only size query (exact workspace size of the transposed-conv cases)",
    "ms_conv1d_parts_launches": "host-only plan query (tests/test_abi.py)",
    "ms_conv1d_parts_workspace_bytes": "host-only size query (exact workspace size of the parts cases)",
    "ms_conv1d_bwd_weight_multi_workspace_bytes": "host-only size query (exact workspace size of the multi cases)",
    "ms_conv1d_kernel_name": "host-only name query (compared with the profile note in the conv cases)",
    "ms_convt1d_kernel_name": "host-only name query",
    "ms_residual_atom_image_bytes": "host-only size query",
    "ms_residual_atom_supported": "host-only geometry query",
    "ms_residual_atom_bwd_supported": "host-only geometry query",
    "ms_residual_atom_publishes_amax": "host-only switch query",
    "ms_residual_atom_sign_words": "host-only size query",
    "ms_residual_stack_supported": "host-only geometry query",
    "ms_residual_stack_signs_supported": "host-only geometry query",
    "ms_conv1d_img_bytes": "host-only size query",
    "ms_conv1d_img_workspace_bytes": "host-only size query",
    "ms_convt1d_img_bytes": "host-only size query",
    "ms_convt1d_img_workspace_bytes": "host-only size query",
    "ms_convt1d_bwd_img_bytes": "host-only size query",
    "ms_convt1d_bwd_img_workspace_bytes": "host-only size query",
    "ms_reduce_workspace_bytes": "host-only size query",
    "ms_l1_mean_multi_workspace_bytes": "host-only size query",
    "ms_l1_mean_multi_fwd_bwd_workspace_bytes": "host-only size query",
    "ms_audio2mel_frames": "host-only geometry query",
    "ms_audio2mel_bwd_workspace_bytes": "host-only size query",
    "ms_stft_frames": "host-only geometry query",
    "ms_stft_mag_bwd_workspace_bytes": "host-only size query",
    "ms_stft_pair_loss_workspace_bytes": "host-only size query",
    "ms_profile_kernels": "profile aid: thread-local host state",
    "ms_profile_take": "profile aid: thread-local host state",
    "ms_debug_install_crash_handler": "debug aid: signal dispositions",
    "ms_comm_unique_id": "comm: host buffer",
    "ms_comm_init": "comm: needs an RCCL communicator (tests/test_gpu_dp.py)",
    "ms_comm_world": "comm: host-only",
    "ms_comm_rank": "comm: host-only",
    "ms_allreduce_f32": "comm: needs an RCCL communicator over several ranks (tests/test_gpu_dp.py)",
    "ms_comm_destroy": "comm: host-only",
    "ms_comm_last_error": "comm: host-only",
}


def test_every_abi_entry_has_a_memory_contract_case():
    from featuresynth._ops import lib as L
    import test_gpu_memcontract as T
    named = set()
    for c in T.CASES:
        assert c.symbols, c.id
        named.update(c.symbols)
    unknown = (named | set(EXEMPT)) - set(L.SIGNATURES)
    assert not unknown, "not in the C ABI: %s" % sorted(unknown)
    both = named & set(EXEMPT)
    assert not both, "exempt AND covered: %s" % sorted(both)
    missing = set(L.SIGNATURES) - named - set(EXEMPT)
    assert not missing, "C-ABI entries without a memory-contract case (tests/test_gpu_memcontract.py) or an EXEMPT reason: %s" \
        % sorted(missing)
    for name, why in EXEMPT.items():
        assert why and (why.startswith(("host-only", "comm", "profile aid", "debug aid"))), name
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids)), "duplicate case ids"
