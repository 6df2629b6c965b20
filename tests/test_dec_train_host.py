"""CPU tests of the decoder's training entry points (include/tpspp_train_dec.h): the header names what it replaces
(tests/test_capi_symbols.py holds it to the binding table and the shared object); argument errors come back as -22 with a
message before anything is launched; the public switches validate their arguments; the decoder refuses on the host what
its HIP training path cannot take; the case tables of tests/test_gpu_dec_train.py hold what they claim."""
import ctypes
import os

import pytest
import torch

import test_gpu_dec_train as TD
from test_attn_train_host import small_recogniser
from tps_pp_amd import NRTRDecoder, _lib, build, losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tpspp_train_dec.h")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def test_header_names_what_it_replaces():
    text = open(HEADER).read()
    assert "replaces:" in text
    for ref in ("nrtr_decoder.py:81-113", "transformer_module.py:24-33,71-96", "ce_loss.py"):
        assert ref in text, ref
    assert "NaN" in text, "the header says what mean over zero scored positions gives"


def _buf():
    b = (ctypes.c_float * 64)()
    return b, ctypes.cast(b, ctypes.c_void_p).value


def fwd(p, q=True, ld_q=128, ld_kv=256, N=1, C=128, heads=2, Tq=20, Tk=30, causal=0, drop_p=0.0, lse=True):
    return (p if q else None, ld_q, p, p, ld_kv, N, C, heads, Tq, Tk, None, None, causal, drop_p, 1, 0, p, p if lse else None,
            None)


def bwd(p, dv=True, ld_q=128, ld_kv=256, N=1, C=128, heads=2, Tq=20, Tk=30, causal=0, drop_p=0.0, ld_dq=128, ld_dkv=256):
    return (p, p, ld_q, p, p, ld_kv, p, p, N, C, heads, Tq, Tk, None, None, causal, drop_p, 1, 0, p, ld_dq, p,
            p if dv else None, ld_dkv, None)


def ce_fwd(p, logits=True, N=1, L=8, K=92, shift=1, red=1, reduced=True):
    return (p if logits else None, L * K, K, 1, p, N, L, K, shift, 92, red, p, p, p if reduced else None, p, None)


def ce_bwd(p, g=True, N=1, L=8, K=92, shift=1, red=1, count=True):
    return (p if g else None, p, L * K, K, 1, p, p, p if count else None, N, L, K, shift, 92, red, p, None)


def test_argument_errors_are_codes_with_messages_and_launch_nothing(lib):
    """Every call below names host memory (or nothing) as its operands: a launch would fail loudly, a -22 launches none.
    N = 0 (M = 0) with good arguments passes the checks and returns before the launch."""
    keep, p = _buf()
    err = lib.tpspp_last_error
    A, B = lib.tpspp_attn_train_fwd_ex, lib.tpspp_attn_train_bwd_ex
    assert A(*fwd(p, N=0)) == 0 and B(*bwd(p, N=0)) == 0
    assert A(*fwd(p, N=0, Tq=256, Tk=256, causal=1)) == 0
    assert lib.tpspp_embed_pos_fwd(p, p, p, 0, 8, 64, 93, p, None) == 0
    assert lib.tpspp_embed_bwd(p, p, 0, 64, 93, 92, p, p, 0, None) == 0
    assert lib.tpspp_seq_ce_fwd(*ce_fwd(p, N=0)) == 0 and lib.tpspp_seq_ce_bwd(*ce_bwd(p, N=0)) == 0
    assert lib.tpspp_embed_bwd_workspace_floats(0, 93, 64) == 0
    assert lib.tpspp_embed_bwd_workspace_floats(513, 93, 64) == 2 * 93 * 64
    # null pointers
    assert A(*fwd(p, q=False)) == -22 and b"null pointer" in err()
    assert A(*fwd(p, lse=False)) == -22 and b"null pointer" in err()
    assert B(*bwd(p, dv=False)) == -22 and b"null pointer" in err()
    assert lib.tpspp_embed_pos_fwd(p, None, p, 1, 8, 64, 93, p, None) == -22 and b"null pointer" in err()
    assert lib.tpspp_embed_bwd(p, p, 8, 64, 93, 92, None, p, 93 * 64, None) == -22 and b"null pointer" in err()
    assert lib.tpspp_seq_ce_fwd(*ce_fwd(p, logits=False)) == -22 and b"null pointer" in err()
    assert lib.tpspp_seq_ce_fwd(*ce_fwd(p, reduced=False)) == -22 and b"null pointer" in err()
    assert lib.tpspp_seq_ce_fwd(*ce_fwd(p, reduced=False, red=0, N=0)) == 0             # none needs no scalar
    assert lib.tpspp_seq_ce_bwd(*ce_bwd(p, g=False)) == -22 and b"null pointer" in err()
    assert lib.tpspp_seq_ce_bwd(*ce_bwd(p, count=False)) == -22 and b"null pointer" in err()
    # C != 64 * heads, a stride below C
    assert A(*fwd(p, C=96)) == -22 and b"64 * heads" in err()
    assert B(*bwd(p, heads=3)) == -22 and b"64 * heads" in err()
    assert A(*fwd(p, ld_q=127)) == -22 and b"row stride" in err()
    assert A(*fwd(p, ld_kv=127)) == -22 and b"row stride" in err()
    assert B(*bwd(p, ld_kv=64)) == -22 and b"row stride" in err()
    assert B(*bwd(p, ld_dq=127)) == -22 and b"row stride" in err()
    assert B(*bwd(p, ld_dkv=127)) == -22 and b"row stride" in err()
    # T above 256
    assert A(*fwd(p, Tq=257)) == -22 and b"256" in err()
    assert A(*fwd(p, Tk=257)) == -22 and b"256" in err()
    assert B(*bwd(p, Tk=257)) == -22 and b"256" in err()
    assert A(*fwd(p, Tq=0)) == -22 and b"bad sizes" in err()
    # drop_p outside [0, 1), causal outside {0, 1}
    for bad in (1.0, -0.1, float("nan")):
        assert A(*fwd(p, drop_p=bad)) == -22 and b"drop_p" in err(), bad
        assert B(*bwd(p, drop_p=bad)) == -22 and b"drop_p" in err(), bad
    for bad in (2, -1):
        assert A(*fwd(p, causal=bad)) == -22 and b"causal" in err(), bad
        assert B(*bwd(p, causal=bad)) == -22 and b"causal" in err(), bad
    # K outside [1, 1024], a bad reduction code, a bad shift
    for bad in (0, 1025):
        assert lib.tpspp_seq_ce_fwd(*ce_fwd(p, K=bad)) == -22 and b"K must lie in [1, 1024]" in err(), bad
        assert lib.tpspp_seq_ce_bwd(*ce_bwd(p, K=bad)) == -22 and b"K must lie in [1, 1024]" in err(), bad
    assert lib.tpspp_seq_ce_fwd(*ce_fwd(p, N=0, K=1024)) == 0 and lib.tpspp_seq_ce_fwd(*ce_fwd(p, N=0, K=1)) == 0
    for bad in (3, -1):
        assert lib.tpspp_seq_ce_fwd(*ce_fwd(p, red=bad)) == -22 and b"reduction" in err(), bad
        assert lib.tpspp_seq_ce_bwd(*ce_bwd(p, red=bad)) == -22 and b"reduction" in err(), bad
    assert lib.tpspp_seq_ce_fwd(*ce_fwd(p, shift=2)) == -22 and b"shift" in err()
    # the embedding's workspace must be large enough
    assert lib.tpspp_embed_bwd(p, p, 8, 64, 93, 92, p, p, 93 * 64 - 1, None) == -22 and b"workspace" in err()
    assert lib.tpspp_embed_pos_fwd(p, p, p, 1, 0, 64, 93, p, None) == -22 and b"bad sizes" in err()
    del keep


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from tps_pp_amd import ops
    q = torch.zeros(1, 4, 64)
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):
        ops.attn_train_autograd_ex(q, q, q, causal=True)
    with pytest.raises(ValueError, match="drop_p"):
        ops.attn_train_autograd_ex(q, q, q, drop_p=1.0)
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):
        ops.embed_pos_autograd(torch.zeros(1, 4, dtype=torch.long), torch.zeros(5, 64), torch.zeros(4, 64))
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):
        ops.seq_cross_entropy_autograd(torch.zeros(1, 4, 5), torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="reduction"):
        ops.seq_cross_entropy_autograd(torch.zeros(1, 4, 5), torch.zeros(1, 4, dtype=torch.long), reduction="avg")


def test_decoder_and_loss_switches_validate_and_default_to_torch():
    dec = NRTRDecoder(n_layers=1, n_head=2, d_model=128, d_embedding=128, d_inner=64)
    loss = losses.TFLoss(ignore_index=92)
    for m in (dec, loss):
        assert m.train_backend == "torch"
        assert m.set_train_backend("hip") is m and m.train_backend == "hip"
        assert m.set_train_backend("torch").train_backend == "torch"
        for bad in ("hip_all", "HIP", None, 1):
            with pytest.raises(ValueError, match='set_train_backend: "torch" or "hip", got'):
                m.set_train_backend(bad)
        assert m.train_backend == "torch"
    # on host logits the loss is PyTorch's under either switch
    logits, targets = torch.randn(2, 8, 92), torch.randint(0, 92, (2, 8))
    a = loss(logits, {"padded_targets": targets})["loss_ce"]
    b = loss.set_train_backend("hip")(logits, {"padded_targets": targets})["loss_ce"]
    assert torch.equal(a, b)


def test_recogniser_switch_passes_the_decoder_and_loss_modes_on():
    m = small_recogniser()
    assert (m.decoder.train_backend, m.loss.train_backend) == ("torch", "torch")
    assert m.set_train_backend("hip_all", backbone="hip", encoder="hip", decoder="hip", loss="hip") is m
    assert (m.encoder.train_backend, m.decoder.train_backend, m.loss.train_backend) == ("hip", "hip", "hip")
    m.set_train_backend("torch")                                   # None leaves them alone
    assert (m.decoder.train_backend, m.loss.train_backend) == ("hip", "hip")
    m.set_train_backend("torch", decoder="torch")
    assert (m.decoder.train_backend, m.loss.train_backend) == ("torch", "hip")
    for bad in ("hip_all", "cuda", 0):
        with pytest.raises(ValueError, match='decoder must be None, "torch" or "hip"'):
            m.set_train_backend("torch", decoder=bad)
        with pytest.raises(ValueError, match='loss must be None, "torch" or "hip"'):
            m.set_train_backend("torch", loss=bad)
    # a failed call changes nothing
    with pytest.raises(ValueError):
        m.set_train_backend("hip", encoder="hip", decoder="hip", loss="nope")
    assert (m.tpsnet.train_backend, m.encoder.train_backend, m.decoder.train_backend) == ("torch", "hip", "torch")
    m.decoder = torch.nn.Identity()
    with pytest.raises(ValueError, match="Identity has no HIP training path"):
        m.set_train_backend("torch", decoder="hip")


def test_decoder_refuses_on_the_host_what_the_hip_path_cannot_take():
    """All on CPU tensors: the refusals come before anything touches a GPU path (which would raise TpsppError)."""
    dec = NRTRDecoder(n_layers=1, n_head=2, d_model=128, d_embedding=128, d_inner=64, num_classes=93, padding_idx=92,
                      start_idx=91, max_seq_len=8).train().set_train_backend("hip")
    enc = torch.zeros(2, 20, 128)
    good = torch.tensor([[91, 3, 4, 91, 92, 92, 92, 92], [91, 5, 91, 92, 92, 92, 92, 92]])
    metas = [dict(valid_ratio=1.0), dict(valid_ratio=0.5)]

    def run(targets, metas=metas, enc=enc):
        return dec(None, enc, {"padded_targets": targets}, metas, train_mode=True)

    bad = good.clone()
    bad[1, 0] = 92
    with pytest.raises(ValueError, match="first token is the padding"):
        run(bad)
    for tok in (93, -1):
        bad = good.clone()
        bad[0, 2] = tok
        with pytest.raises(ValueError, match=r"target tokens must lie in \[0, 93\)"):
            run(bad)
    with pytest.raises(ValueError, match="mask length 0"):
        run(good, [dict(valid_ratio=1.0), dict(valid_ratio=0.0)])
    with pytest.raises(ValueError, match="at most 256 encoder tokens"):
        run(good, enc=torch.zeros(2, 257, 128))
    with pytest.raises(ValueError, match="1 to 256 target positions"):
        run(torch.full((2, 257), 91))
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):          # good arguments reach the (absent) GPU path
        run(good)


# ---- the case tables of the GPU tests ------------------------------------------------------------------------------------
def test_cross_entropy_cases_have_a_scored_position_except_the_one_that_tests_zero_over_zero():
    names = [c["name"] for c in TD.CE_CASES]
    assert len(set(names)) == len(names)
    for c in TD.CE_CASES:
        assert (TD.ce_scored(c) == 0) == (c["name"] == "all-ignored"), c["name"]
    assert {c["K"] for c in TD.CE_CASES} >= {1, 5, 92, 1024} and {c["L"] for c in TD.CE_CASES} >= {2, 8, 40}
    assert {c["shift"] for c in TD.CE_CASES} == {True, False}
    # an image with all targets ignored next to images with scored positions; logits of +-80
    c = TD.CE_BY_NAME["K92-L40-shift"]
    _, t = TD.ce_inputs(c)
    assert (t[1] == TD.CE_IGNORE).all() and TD.ce_scored(c) > 0
    x, _ = TD.ce_inputs(TD.CE_BY_NAME["K92-big"])
    assert (x == 80).any() and (x == -80).any()
    # the float64 reference alone: finite wherever a position is scored, NaN for the mean over none
    for c in TD.CE_CASES:
        loss, d = TD.ce_run(c, "mean", True, torch.float64, "cpu")
        assert torch.isnan(loss) == (c["name"] == "all-ignored") and torch.isfinite(d).all(), c["name"]


def test_attention_cases_document_their_empty_rows():
    assert {c["Tq"] for c in TD.SELF_CASES} >= {1, 8, 40, 64, 65, 130}
    assert [(c["Tq"], c["Tk"]) for c in TD.CROSS_CASES] == [(1, 20), (8, 20), (3, 1), (40, 64), (40, 65), (65, 256)]
    for c in TD.SELF_CASES + TD.CROSS_CASES:
        vis = TD.visible(c)
        assert vis.shape[0] <= 3 and c["heads"] in (1, 2), c["name"]
        empty = ~vis.any(-1)
        want = torch.zeros_like(empty)
        for b, rows in c["empty_rows"].items():
            want[b, rows] = True
        assert torch.equal(empty, want), f"{c['name']}: the rows that see no key are not the documented ones"
        # the float64 reference is finite everywhere but the lse of the empty rows
        q, k, v, gout = TD.make_case(c)
        res = TD.ref_run((q, k, v), gout, c["heads"], vis, torch.float64, "cpu")
        assert all(torch.isfinite(t).all() for t in [res[0]] + res[2:]), c["name"]
        assert torch.equal(torch.isinf(res[1]), empty[:, None, :].expand_as(res[1])), c["name"]
        for b, rows in c["empty_rows"].items():
            assert (res[0][b, rows] == 0).all() and (res[2][b, rows] == 0).all()
    # T = 130: a query that sees block 0, nothing in block 1 and block 2
    vis = TD.visible(TD.ATTN_CASES["T130"])[1]
    assert vis[129, :64].all() and not vis[129, 64:128].any() and vis[129, 128]
    assert any(c["empty_rows"] for c in TD.SELF_CASES)
    for c in TD.CROSS_CASES:
        vl = c["valid_len"]
        assert 1 in vl and max(vl) == c["Tk"] and (c["Tk"] - 1) // 64 == (vl[2] - 1) // 64 or c["Tk"] in (1, 65), c["name"]
    # pad suffix and pads in the middle
    km = TD.ATTN_CASES["T40"]["key_mask"]
    assert km[0].all() and not km[1, 17:].any() and km[1, :17].all() and km[2, :9].all() and km[2, 21:].all()
