"""CPU tests of the encoder's attention training entry points (include/tpspp_train_attn.h): the header names what it
replaces (tests/test_capi_symbols.py holds it to the binding table and the shared object); argument errors come back as -22
with a message before anything is launched; the public switches validate their arguments."""
import ctypes
import os

import pytest
import torch

from tps_pp_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tpspp_train_attn.h")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def test_header_names_what_it_replaces():
    assert "replaces:" in open(HEADER).read() and "transformer_module.py:24-33,71-96" in open(HEADER).read()


def _buf():
    b = (ctypes.c_float * 64)()
    return b, ctypes.cast(b, ctypes.c_void_p).value


def fwd_args(p, q=True, ld=128, N=1, C=128, heads=2, Tq=20, Tk=20, drop_p=0.0, out=True):
    return (p if q else None, p, p, ld, N, C, heads, Tq, Tk, None, drop_p, 1, 0, p if out else None, p, None)


def bwd_args(p, dq=True, ld=128, N=1, C=128, heads=2, Tq=20, Tk=20, drop_p=0.0, ldg=128):
    return (p, p, p, p, ld, p, p, N, C, heads, Tq, Tk, None, drop_p, 1, 0, p if dq else None, p, p, ldg, None)


def test_argument_errors_are_codes_with_messages_and_launch_nothing(lib):
    """Every call below names host memory (or nothing) as its operands: a launch would fail loudly, a -22 launches none.
    N = 0 with good arguments is the only call that passes the checks, and it returns before the launch."""
    keep, p = _buf()
    err = lib.tpspp_last_error
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, N=0)) == 0
    assert lib.tpspp_attn_train_bwd(*bwd_args(p, N=0)) == 0
    assert lib.tpspp_attn_dropout_mask(0, 2, 20, 20, 0.5, 1, 0, p, None) == 0
    # null pointers
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, q=False)) == -22 and b"null pointer" in err()
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, out=False)) == -22 and b"null pointer" in err()
    assert lib.tpspp_attn_train_bwd(*bwd_args(p, dq=False)) == -22 and b"null pointer" in err()
    assert lib.tpspp_attn_dropout_mask(1, 2, 20, 20, 0.5, 1, 0, None, None) == -22 and b"null pointer" in err()
    # C != 64 * heads, rows closer than C
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, C=96, ld=96)) == -22 and b"64 * heads" in err()
    assert lib.tpspp_attn_train_bwd(*bwd_args(p, heads=3)) == -22 and b"64 * heads" in err()
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, ld=127)) == -22 and b"row stride" in err()
    assert lib.tpspp_attn_train_bwd(*bwd_args(p, ldg=64)) == -22 and b"row stride" in err()
    # T = 257 (256 passes the check: N = 0 keeps it from launching)
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, Tq=257, Tk=257)) == -22 and b"256" in err()
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, Tk=257)) == -22 and b"256" in err()
    assert lib.tpspp_attn_train_bwd(*bwd_args(p, Tq=257)) == -22 and b"256" in err()
    assert lib.tpspp_attn_dropout_mask(1, 2, 257, 20, 0.5, 1, 0, p, None) == -22 and b"256" in err()
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, N=0, Tq=256, Tk=256)) == 0
    assert lib.tpspp_attn_train_fwd(*fwd_args(p, Tq=0)) == -22 and b"bad sizes" in err()
    # drop_p outside [0, 1)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        assert lib.tpspp_attn_train_fwd(*fwd_args(p, drop_p=bad)) == -22 and b"drop_p" in err(), bad
        assert lib.tpspp_attn_train_bwd(*bwd_args(p, drop_p=bad)) == -22 and b"drop_p" in err(), bad
        assert lib.tpspp_attn_dropout_mask(1, 2, 20, 20, bad, 1, 0, p, None) == -22 and b"drop_p" in err(), bad
    del keep


def test_ops_refuse_cpu_tensors_and_bad_rates():
    from tps_pp_amd import ops
    q = torch.zeros(1, 4, 64)
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):
        ops.attn_train_autograd(q, q, q)
    with pytest.raises(ValueError, match="drop_p"):
        ops.attn_train_autograd(q, q, q, drop_p=1.0)
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):
        ops.attn_dropout_mask(1, 1, 4, 4, 0.5, 1, 0, "cpu")


def test_both_autograd_names_raise_the_same_rate_error():
    from tps_pp_amd import ops
    q = torch.zeros(1, 4, 64)
    with pytest.raises(ValueError) as old:
        ops.attn_train_autograd(q, q, q, drop_p=1.0)
    with pytest.raises(ValueError) as new:
        ops.attn_train_autograd_ex(q, q, q, drop_p=1.0)
    assert type(old.value) is type(new.value) is ValueError and str(old.value) == str(new.value)
    assert "drop_p must lie in [0, 1), got 1.0" in str(old.value)


def _switchable(name):
    import tps_pp_amd as P
    from tps_pp_amd import losses
    return {"TPS_PP": lambda: P.TPS_PP(),
            "ResNetABI_v2_large": lambda: P.ResNetABI_v2_large(arch_settings=[1, 1, 1, 1, 1], strides=[2, 1, 2, 1, 2]),
            "NRTREncoder": lambda: P.NRTREncoder(n_layers=1, n_head=2, d_model=128, d_inner=64),
            "NRTRDecoder": lambda: P.NRTRDecoder(n_layers=1, n_head=2, d_model=128, d_embedding=128, d_inner=64),
            "_SequenceLoss": lambda: losses._SequenceLoss(92, "none", shift=True, flatten=True)}[name]()


@pytest.mark.parametrize("name", ["TPS_PP", "ResNetABI_v2_large", "NRTREncoder", "NRTRDecoder", "_SequenceLoss"])
def test_the_five_train_backend_switches_are_one(name):
    from tps_pp_amd.registry import TrainBackendMixin
    m = _switchable(name)
    modes = ("torch", "hip", "hip_all") if name == "TPS_PP" else ("torch", "hip")
    text = '"torch", "hip" or "hip_all"' if name == "TPS_PP" else '"torch" or "hip"'
    assert isinstance(m, TrainBackendMixin) and type(m).TRAIN_BACKENDS == modes
    assert "train_backend" not in vars(type(m))                # the property is the mixin's
    assert m.train_backend == "torch"
    for mode in modes[::-1]:
        assert m.set_train_backend(mode) is m and m.train_backend == mode
    for bad in ("x", "HIP", "hip_some", None, 1) + (() if name == "TPS_PP" else ("hip_all",)):
        with pytest.raises(ValueError) as e:
            m.set_train_backend(bad)
        assert str(e.value) == f"set_train_backend: {text}, got {bad!r}"
        assert m.train_backend == "torch"                      # modes[::-1] ended on "torch": the old value stays
    m.set_train_backend("hip")
    with pytest.raises(ValueError):
        m.set_train_backend("x")
    assert m.train_backend == "hip"
    # an object built before the attribute existed reads as "torch"
    del m._train_backend
    assert m.train_backend == "torch"
    # what each mode means for this class is still written down
    doc = (type(m).set_train_backend.__doc__ or "") + (type(m).__doc__ or "")
    assert '"hip"' in doc and '"torch"' in doc


def small_recogniser(**kw):
    import tps_pp_amd as P
    return P.build_detector(dict(type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1],
                                                            strides=[2, 1, 2, 1, 2]),
                                 tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1),
                                 decoder=dict(type="NRTRDecoder", n_layers=1), loss=dict(type="TFLoss"),
                                 label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
                                 max_seq_len=8, **kw))


def test_encoder_switch_validates_and_defaults_to_torch():
    from tps_pp_amd import NRTREncoder
    enc = NRTREncoder(n_layers=1, n_head=2, d_model=128, d_inner=64)
    assert enc.train_backend == "torch"
    assert enc.set_train_backend("hip") is enc and enc.train_backend == "hip"
    assert enc.set_train_backend("torch").train_backend == "torch"
    for bad in ("hip_all", "HIP", None, 1):
        with pytest.raises(ValueError, match='set_train_backend: "torch" or "hip", got'):
            enc.set_train_backend(bad)
    assert enc.train_backend == "torch"
    # the HIP training path has no CPU form either
    enc.set_train_backend("hip").train()
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):
        enc(torch.zeros(1, 128, 1, 4))


def test_recogniser_switch_passes_the_encoder_mode_on():
    m = small_recogniser()
    assert m.encoder.train_backend == "torch"
    assert m.set_train_backend("hip_all", backbone="hip", encoder="hip") is m
    assert (m.tpsnet.train_backend, m.backbone.train_backend, m.encoder.train_backend) == ("hip_all", "hip", "hip")
    m.set_train_backend("torch")                                   # encoder=None (and backbone=None) leave them alone
    assert (m.tpsnet.train_backend, m.backbone.train_backend, m.encoder.train_backend) == ("torch", "hip", "hip")
    m.set_train_backend("torch", encoder="torch")
    assert m.encoder.train_backend == "torch" and m.backbone.train_backend == "hip"
    for bad in ("hip_all", "cuda", 0):
        with pytest.raises(ValueError, match='encoder must be None, "torch" or "hip"'):
            m.set_train_backend("torch", encoder=bad)
    assert m.encoder.train_backend == "torch"
    # a failed call changes nothing, whichever argument is wrong
    with pytest.raises(ValueError):
        m.set_train_backend("hip", backbone="torch", encoder="nope")
    assert (m.tpsnet.train_backend, m.backbone.train_backend) == ("torch", "hip")
    # an encoder without the method raises as the backbone case does
    m.encoder = torch.nn.Identity()
    with pytest.raises(ValueError, match="Identity has no HIP training path"):
        m.set_train_backend("torch", encoder="hip")
    m.set_train_backend("hip", encoder=None)
    assert m.tpsnet.train_backend == "hip"
