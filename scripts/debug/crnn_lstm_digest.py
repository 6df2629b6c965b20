"""One sha256 per output tensor of the six CRNN LSTM entry points, every precision mode, on inputs built from an integer hash
of the element index (no RNG: the same anywhere).  Two builds of the library compute the same bits exactly when their
listings are identical -- run it once per build (scripts/debug/lib_ab.sh swaps the .so).
python scripts/debug/crnn_lstm_digest.py"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tps_pp_amd import ops  # noqa: E402

H = ops.CRNN_HIDDEN
dev = torch.device("cuda:0")


def unit(shape, salt):
    """(0, 1) on a grid of 2^-16, exact in fp32: a 32-bit mix of the element index."""
    n = 1
    for s in shape:
        n *= s
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + salt * 40503 + 12345) & 0xffffffff
    h = ((h ^ (h >> 15)) * 2246822519) & 0xffffffff
    h = ((h ^ (h >> 13)) * 3266489917) & 0xffffffff
    h = (h ^ (h >> 16)) & 0xffff
    return ((h.double() + 0.5) / 65536.0).float().reshape(shape)


def sym(shape, salt, scale):
    return (unit(shape, salt) * 2.0 - 1.0) * scale


def digest(label, t):
    print(f"{label:58s} {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}")


w_hh = sym((2, 4 * H, H), 1, 0.0625).to(dev)
w_hh_t = w_hh.transpose(1, 2).contiguous()
for T in (1, 2, 26):
    for N in (5, 17):
        xg, d_out = sym((T, N, 2, 4 * H), 2, 2.0).to(dev), sym((T, N, 2 * H), 3, 1.0).to(dev)
        gates = unit((T, N, 2, 4 * H), 4)                                       # i, f, o in (0, 1), g in (-1, 1)
        gates[..., 2 * H:3 * H] = gates[..., 2 * H:3 * H] * 2.0 - 1.0
        gates, cell = gates.to(dev), sym((T, N, 2, H), 5, 2.0).to(dev)
        for g in (0, 16):
            at = f"T={T} N={N} g={g}"
            digest(f"lstm_fwd out {at}", ops.crnn_lstm(xg, w_hh, g))
            for name, t in zip(("out", "gates", "cell"), ops.crnn_lstm_train_fwd(xg, w_hh, g)):
                digest(f"lstm_train_fwd {name} {at}", t)
            for name, t in zip(("d_xg", "d_xg_dir"), ops.crnn_lstm_bwd(d_out, gates, cell, w_hh_t, g, direction_major=True)):
                digest(f"lstm_bwd {name} {at}", t)
            for x3 in (False, True):
                mode = "bf16x3" if x3 else "bf16"
                mw, mw_t = ops.arrange_mfma16(w_hh, x3=x3), ops.arrange_mfma16(w_hh_t, x3=x3)
                digest(f"lstm_bf16_fwd {mode} out {at}", ops.crnn_lstm_bf16(xg, mw, g))
                for name, t in zip(("out", "gates", "cell"), ops.crnn_lstm_bf16_train_fwd(xg, mw, g)):
                    digest(f"lstm_bf16_train_fwd {mode} {name} {at}", t)
                digest(f"lstm_bf16_bwd {mode} d_xg {at}", ops.crnn_lstm_bf16_bwd(d_out, gates, cell, mw_t, g))
