"""Inputs and weights of the CRNN fixtures (crnn_tps.npz), shared by make_crnn_golden.py and the tests: values only, from
`tps_pp_amd.synth`, so that the tests rebuild them without reading the reference."""
import json
import os

import numpy as np

from tps_pp_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))

SEED = 0                                  # make_crnn_golden.py asserts the top-2 logit margin this seed gives (>= MARGIN)
MARGIN = 1e-3
N, HW = 3, (32, 100)                      # crnn_tps.py's geometry: T = 26
N32, HW32 = 2, (32, 32)                   # the narrow case without a preprocessor: T = 9
VALID_RATIOS = (1.0, 0.5, 0.27)
TEXTS = ["hello", "Tps", "crnn2016"]     # lower=True folds the capital
TOPK = 3
KEEP = ("preprocessor.LocalizationNetwork.localization_fc2.bias", "preprocessor.GridGenerator.inv_delta_C",
        "preprocessor.GridGenerator.P_hat")


def models():
    """{'crnn_tps': model dict of configs/_base_/recog_models/crnn_tps.py, 'crnn': of crnn.py} (crnn_models.json; JSON turns
    the size tuples into lists: `TPSPreprocessor` asserts tuples, so they are turned back)."""
    with open(os.path.join(HERE, "crnn_models.json")) as f:
        d = json.load(f)
    for m in d.values():
        pre = m.get("preprocessor")
        if pre:
            for k in ("img_size", "rectified_img_size"):
                pre[k] = tuple(pre[k])
    return d


def images():
    return synth.smooth_image((N, 1) + HW, "crnn.img", SEED)


def images32():
    return synth.smooth_image((N32, 1) + HW32, "crnn.img32", SEED)


def state_rule(name, shape):
    if name.endswith("running_var"):
        return (0.25, 1.0)                # in [0.75, 1.25)
    if name.endswith("running_mean"):
        return (0.1, 0.0)
    if name.endswith("localization_fc2.weight"):
        return (0.02, 0.0)                # non-zero, and C' stays near the initial lattice
    if len(shape) == 1 and name.endswith(".weight") and ("batchnorm" in name or "LocalizationNetwork.conv." in name):
        return (0.25, 1.0)                # BatchNorm gamma
    if ".rnn.weight" in name or ".embedding.weight" in name:
        return (2.0 / np.sqrt(shape[1]), 0.0)      # twice the fan-in scale: logits that differ between positions
    return None


def state(module_state, seed=SEED):
    """name -> fp32 array for every float tensor of the model's state_dict except KEEP and num_batches_tracked."""
    shapes = {k: tuple(v.shape) for k, v in module_state.items() if k not in KEEP and not k.endswith("num_batches_tracked")}
    return synth.state_dict_like(shapes, seed, state_rule)


def img_metas(n, ratios=None):
    return [dict(valid_ratio=float(ratios[i])) if ratios is not None else {} for i in range(n)]
