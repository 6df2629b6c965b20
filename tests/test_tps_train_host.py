"""CPU tests of the classic rectifier's "hip" train backend: the argument checks of the entry points of
tpspp_bn_pool_train.hip on host pointers (nothing is launched), the workspace formula, the float64 restatement of the
header's backward formulas against PyTorch's autograd, and the backend switch of TPSPreprocessor and the recognisers."""
import ctypes

import pytest
import torch

import tps_train_cases as cases
from tps_pp_amd import TPSPreprocessor, _lib, build, build_detector

vp, ci = ctypes.c_void_p, ctypes.c_int


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def host():
    buf = (ctypes.c_float * 4096)()
    return buf, ctypes.cast(buf, vp).value


def refused(lib, rc, *words):
    msg = lib.tpspp_last_error().decode()
    assert rc == -22, (rc, msg)
    for w in words:
        assert w in msg, msg


# ---- argument checks --------------------------------------------------------------------------------------------------------
def test_fwd_argument_checks(lib, host):
    _, p = host
    good = [p, p, p, p, p, 0, 3, 4, 4, p, None]              # N = 0: every check runs, nothing is launched
    assert lib.tpspp_bn_pool2x2_fwd(*good) == 0
    for i in (0, 1, 2, 3, 4, 9):
        bad = list(good); bad[i] = None
        refused(lib, lib.tpspp_bn_pool2x2_fwd(*bad), "tpspp_bn_pool2x2_fwd", "null pointer")
    for i, v in ((7, 1), (8, 1), (6, 0), (6, -1), (5, -1), (6, 65536)):
        bad = list(good); bad[i] = v
        refused(lib, lib.tpspp_bn_pool2x2_fwd(*bad), "tpspp_bn_pool2x2_fwd")
    bad = list(good); bad[5:9] = [1 << 12, 1 << 10, 1 << 5, 1 << 5]      # 2^32 elements
    refused(lib, lib.tpspp_bn_pool2x2_fwd(*bad), "2^31")


def test_bwd_reduce_argument_checks(lib, host):
    _, p = host
    good = [p, p, p, p, p, p, 0, 3, 4, 4, p, p, None, 0, None]
    assert lib.tpspp_bn_pool2x2_bwd_reduce(*good) == 0
    for i in (0, 1, 2, 3, 4, 5, 10, 11):
        bad = list(good); bad[i] = None
        refused(lib, lib.tpspp_bn_pool2x2_bwd_reduce(*bad), "tpspp_bn_pool2x2_bwd_reduce", "null pointer")
    for i, v in ((8, 1), (9, 1), (7, 0), (7, -2), (6, -1)):
        bad = list(good); bad[i] = v
        refused(lib, lib.tpspp_bn_pool2x2_bwd_reduce(*bad), "bad sizes")
    # a short workspace, and a NULL one, with a real batch: refused before any launch
    need = lib.tpspp_bn_pool2x2_bwd_reduce_workspace_floats(2, 3, 4, 4)
    assert need == 6
    bad = list(good); bad[6] = 2; bad[12] = p; bad[13] = need - 1
    refused(lib, lib.tpspp_bn_pool2x2_bwd_reduce(*bad), "ws too small", "6 floats")
    bad[12] = None; bad[13] = need
    refused(lib, lib.tpspp_bn_pool2x2_bwd_reduce(*bad), "ws too small")


def test_bwd_data_argument_checks(lib, host):
    _, p = host
    good = [p, p, p, p, p, p, p, p, 1, 0, 3, 4, 4, p, None]
    assert lib.tpspp_bn_pool2x2_bwd_data(*good) == 0
    for i in (0, 1, 2, 3, 4, 5, 13):
        bad = list(good); bad[i] = None
        refused(lib, lib.tpspp_bn_pool2x2_bwd_data(*bad), "tpspp_bn_pool2x2_bwd_data", "null pointer")
    for v in (-1, 2):
        bad = list(good); bad[8] = v
        refused(lib, lib.tpspp_bn_pool2x2_bwd_data(*bad), "train must be 0 or 1")
    for i in (6, 7):                                            # train = 1 without a sum
        bad = list(good); bad[i] = None
        refused(lib, lib.tpspp_bn_pool2x2_bwd_data(*bad), "train = 1 needs sum_dr")
        bad[8] = 0                                              # train = 0: the sums may be NULL
        assert lib.tpspp_bn_pool2x2_bwd_data(*bad) == 0
    for i, v in ((11, 1), (12, 1), (10, 0), (9, -1)):
        bad = list(good); bad[i] = v
        refused(lib, lib.tpspp_bn_pool2x2_bwd_data(*bad), "bad sizes")


def test_global_avgpool_bwd_argument_checks(lib, host):
    _, p = host
    good = [p, 0, 3, 4, 4, p, None]
    assert lib.tpspp_global_avgpool_bwd(*good) == 0
    for i in (0, 5):
        bad = list(good); bad[i] = None
        refused(lib, lib.tpspp_global_avgpool_bwd(*bad), "tpspp_global_avgpool_bwd", "null pointer")
    for i, v in ((1, -1), (2, 0), (3, 0), (4, 0)):
        bad = list(good); bad[i] = v
        refused(lib, lib.tpspp_global_avgpool_bwd(*bad), "bad sizes")


def test_workspace_query_against_its_formula(lib):
    for N, C, H, W in cases.CASES + [(512, 64, 32, 100), (1, 1, 64, 64), (1, 1, 64, 65), (7, 3, 2, 3)]:
        S = (N * H * W + 4095) // 4096
        assert lib.tpspp_bn_pool2x2_bwd_reduce_workspace_floats(N, C, H, W) == S * C * 2, (N, C, H, W)
    for dims in ((0, 3, 4, 4), (2, 0, 4, 4), (2, 3, 0, 4), (2, 3, 4, -1)):
        assert lib.tpspp_bn_pool2x2_bwd_reduce_workspace_floats(*dims) == 0
    # (3, 8, 37, 41) is the two-slice case the table promises
    assert lib.tpspp_bn_pool2x2_bwd_reduce_workspace_floats(3, 8, 37, 41) == 2 * 8 * 2


# ---- the cases and the restated formulas --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_a_well_separated_seed_exists_and_has_the_three_channels(case):
    c = cases.make_case(*case)
    assert 0 <= c["seed"] < cases.MAX_SEEDS
    z, gamma, beta = c["z"], c["gamma"], c["beta"]
    assert torch.equal(z * 64, torch.round(z * 64))                                   # dyadic grid
    assert gamma[0] < 0 and bool((z[:, 1] == z[0, 1, 0, 0]).all()) and beta[1] > 0
    assert abs(float(z[:, 2].double().mean()) - 1e3) < 1
    # negative gamma: the pooled activation of channel 0 comes from the minimum of z in its window
    mean, rstd = cases.batch_stats(z)
    a4 = cases.windows(cases.activation(z.double(), mean, rstd, gamma.double(), beta.double()))[:, 0]
    z4 = cases.windows(z.double())[:, 0]
    m, k = cases.scan(a4)
    pos = m > 0
    assert bool((z4.gather(-1, k.unsqueeze(-1)).squeeze(-1)[pos] == z4.min(-1).values[pos]).all())
    # the constant channel: every window a tie, the first element selected
    _, k1 = cases.scan(cases.windows(cases.activation(z.double(), mean, rstd, gamma.double(), beta.double()))[:, 1])
    assert bool((k1 == 0).all())


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_restated_formulas_against_float64_autograd(case, train):
    c = cases.make_case(*case)
    ref = cases.autograd_reference(*case, train)
    z = c["z"].double()
    mean, rstd = cases.batch_stats(z) if train else cases.eval_stats(c["running_mean"], c["running_var"])
    p, dz, sdr, sdx = cases.restated_backward(z, c["dp"].double(), mean, rstd, c["gamma"].double(), c["beta"].double(), train)
    for name, got, want in (("p", p, ref["p"]), ("dz", dz, ref["dz"]), ("dbeta", sdr, ref["dbeta"]),
                            ("dgamma", sdx, ref["dgamma"])):
        scale = max(1.0, float(want.abs().max()))
        assert float((got - want).abs().max()) <= 1e-12 * scale, (name, float((got - want).abs().max()), scale)
    H, W = case[2:]
    if not train:                       # the row / column no window covers gets no gradient
        assert bool((dz[:, :, 2 * (H // 2):] == 0).all()) and bool((dz[:, :, :, 2 * (W // 2):] == 0).all())


# ---- the switch -------------------------------------------------------------------------------------------------------------
def crnn_tps():
    return build_detector(dict(
        type="CRNNNet", preprocessor=dict(type="TPSPreprocessor", num_fiducial=20, img_size=(32, 100),
                                          rectified_img_size=(32, 100), num_img_channel=1),
        backbone=dict(type="VeryDeepVgg", leaky_relu=False, input_channels=1), encoder=None,
        decoder=dict(type="CRNNDecoder", in_channels=512, rnn_flag=True), loss=dict(type="CTCLoss"),
        label_convertor=dict(type="CTCConvertor", dict_type="DICT36", with_unknown=False, lower=True)))


def nrtr_tpspp():
    return build_detector(dict(
        type="NRTR", backbone=dict(type="ResNetABI_v2_large", arch_settings=[1, 1, 1, 1, 1], strides=[2, 1, 2, 1, 2]),
        tpsnet=dict(type="TPS_PP"), encoder=dict(type="NRTREncoder", n_layers=1), decoder=dict(type="NRTRDecoder", n_layers=1),
        loss=dict(type="TFLoss"), label_convertor=dict(type="AttnConvertor", dict_type="DICT90", with_unknown=True),
        max_seq_len=8))


def test_switch_default_modes_and_state_dict():
    m = TPSPreprocessor(20, (32, 100), (32, 100), 1)
    keys = list(m.state_dict())
    assert m.train_backend == "torch"
    assert m.set_train_backend("hip") is m and m.train_backend == "hip"
    for bad in ("HIP", "hip_all", None, 1):
        with pytest.raises(ValueError, match="set_train_backend"):
            m.set_train_backend(bad)
        assert m.train_backend == "hip"
    assert list(m.state_dict()) == keys
    assert m.set_train_backend("torch").train_backend == "torch"
    assert m.set_train_io_dtype(torch.bfloat16).set_train_backend("hip").train_io_dtype == torch.bfloat16


def test_recogniser_switch_reaches_the_preprocessor():
    m = crnn_tps()
    keys = list(m.state_dict())
    assert m.preprocessor.train_backend == "torch"
    m.set_train_backend("torch", preprocessor="hip", decoder="hip", loss="hip")
    assert (m.preprocessor.train_backend, m.decoder.train_backend, m.loss.train_backend) == ("hip", "hip", "hip")
    assert list(m.state_dict()) == keys
    # a call that fails changes nothing: the VGG has no HIP training path, a bad value is refused
    with pytest.raises(ValueError, match="has no HIP training path"):
        m.set_train_backend("torch", preprocessor="torch", decoder="torch", backbone="hip")
    with pytest.raises(ValueError, match="preprocessor must be None"):
        m.set_train_backend("torch", decoder="torch", preprocessor="HIP")
    assert (m.preprocessor.train_backend, m.decoder.train_backend, m.loss.train_backend) == ("hip", "hip", "hip")
    m.set_train_backend("torch", preprocessor="torch")
    assert m.preprocessor.train_backend == "torch" and m.decoder.train_backend == "hip"
    m.set_train_backend("torch")                                # None leaves a part as it is
    assert m.preprocessor.train_backend == "torch" and m.decoder.train_backend == "hip"


def test_a_model_without_the_classic_rectifier_refuses_the_keyword():
    m = nrtr_tpspp()
    before = (m.backbone.train_backend, m.encoder.train_backend, m.tpsnet.train_backend)
    with pytest.raises(ValueError, match="has no HIP training path"):
        m.set_train_backend("hip", backbone="hip", preprocessor="hip")
    assert (m.backbone.train_backend, m.encoder.train_backend, m.tpsnet.train_backend) == before
