"""Training step of the NRTR decoder and its loss on both train backends, in one process (needs an MI355X; fails without a
GPU).

    python scripts/bench_decoder_train.py [--batch 512] [--tokens 64] [--len 40] [--layers 6] [--reps 7] [--iters 5]
                                          [--out FILE]

Shape: the recogniser's own (6 layers, d_model 512, d_inner 256, 8 heads, 93 classes) against T = 64 encoder tokens and
L = 40 target positions per image.  For dropout 0.1 and 0.0 it reports
  * ms per forward + backward of the decoder + TFLoss (mean) for "torch" and "hip": after a warm-up of each, `reps` timed
    regions of `iters` steps per backend, the two backends alternating region by region, device events around each region,
    median and min / max of the per-step times;
  * the new entry points' own call times at the same shape (device events around isolated calls, median over `reps`
    regions): causal self-attention and cross-attention forward and backward, the embedding forward and backward, the
    cross-entropy forward and backward.
One JSON line per dropout rate."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tps_pp_amd import NRTRDecoder, losses, ops  # noqa: E402
from bench_encoder_train import summary, timed  # noqa: E402

CLASSES, PAD, START = 93, 92, 91


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--len", type=int, default=40)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decoder_train: no GPU (there is no CPU form of this measurement)")
    dev = torch.device("cuda:0")
    N, T, L, C, heads = a.batch, a.tokens, a.len, 512, 8
    g = torch.Generator().manual_seed(0)
    targets = torch.full((N, L), PAD, dtype=torch.long)
    for b in range(N):                       # <SOS>, 3 .. L - 2 characters, <EOS>, padding
        n = 3 + (7 * b) % (L - 4)
        targets[b, 0], targets[b, n + 1] = START, START
        targets[b, 1:n + 1] = torch.randint(0, 90, (n,), generator=g)
    tdict = {"padded_targets": targets}
    metas = [dict(valid_ratio=1.0 if i % 2 else 0.8) for i in range(N)]
    lines = []
    for p in (0.1, 0.0):
        torch.manual_seed(0)
        dec = NRTRDecoder(n_layers=a.layers, d_model=C, d_inner=256, n_head=heads, dropout=p, num_classes=CLASSES,
                          start_idx=START, padding_idx=PAD, max_seq_len=L).to(dev).train()
        loss = losses.TFLoss(ignore_index=PAD, reduction="mean")
        out_enc = torch.randn((N, T, C), device=dev, requires_grad=True)

        def step(mode):
            def run():
                dec.set_train_backend(mode)
                loss.set_train_backend(mode)
                for q in dec.parameters():
                    q.grad = None
                out_enc.grad = None
                loss(dec(None, out_enc, tdict, metas, train_mode=True), tdict)["loss_ce"].backward()
            return run

        steps = {m: step(m) for m in ("torch", "hip")}
        for m in steps:                      # warm-up: code objects, allocator, library algorithm choices
            timed(steps[m], 3)
        times = {m: [] for m in steps}
        for _ in range(a.reps):              # alternate the backends region by region
            for m in steps:
                times[m].append(timed(steps[m], a.iters))

        # the new entry points by themselves, on one layer's operands
        tok = targets.to(dev).int()
        km = (tok != PAD).view(torch.uint8)
        vl = torch.tensor([T if i % 2 else int(0.8 * T) for i in range(N)], dtype=torch.int32, device=dev)
        qkv, dqkv = torch.randn((N * L, 3 * C), device=dev), torch.empty((N * L, 3 * C), device=dev)
        qp, dqp = torch.randn((N * L, C), device=dev), torch.empty((N * L, C), device=dev)
        kv, dkv = torch.randn((N * T, 2 * C), device=dev), torch.empty((N * T, 2 * C), device=dev)
        dout = torch.randn((N * L, C), device=dev)
        so, sl = ops.attn_train_fwd_ex(qkv, 3 * C, qkv[:, C:], qkv[:, 2 * C:], 3 * C, N, C, heads, L, L, None, km, True, p, 1, 0)
        co, cl = ops.attn_train_fwd_ex(qp, C, kv, kv[:, C:], 2 * C, N, C, heads, L, T, vl, None, False, p, 1, 1)
        emb, pos = torch.randn((CLASSES, C), device=dev), torch.randn((L, C), device=dev)
        dx = torch.randn((N * L, C), device=dev)
        logits = torch.randn((N, L, CLASSES - 1), device=dev)
        _, lse, _, cnt = ops.seq_ce_fwd(logits, tok, True, PAD, 1)
        one = torch.ones((1,), device=dev)
        calls = dict(
            self_attn_fwd=lambda: ops.attn_train_fwd_ex(qkv, 3 * C, qkv[:, C:], qkv[:, 2 * C:], 3 * C, N, C, heads, L, L, None,
                                                        km, True, p, 1, 0),
            self_attn_bwd=lambda: ops.attn_train_bwd_ex(dout, qkv, 3 * C, qkv[:, C:], qkv[:, 2 * C:], 3 * C, so, sl, N, C, heads,
                                                        L, L, None, km, True, p, 1, 0, dqkv, 3 * C, dqkv[:, C:],
                                                        dqkv[:, 2 * C:], 3 * C),
            cross_attn_fwd=lambda: ops.attn_train_fwd_ex(qp, C, kv, kv[:, C:], 2 * C, N, C, heads, L, T, vl, None, False, p, 1,
                                                         1),
            cross_attn_bwd=lambda: ops.attn_train_bwd_ex(dout, qp, C, kv, kv[:, C:], 2 * C, co, cl, N, C, heads, L, T, vl, None,
                                                         False, p, 1, 1, dqp, C, dkv, dkv[:, C:], 2 * C),
            embed_fwd=lambda: ops.embed_pos_fwd(tok, emb, pos),
            embed_bwd=lambda: ops.embed_bwd(dx, tok, CLASSES, PAD),
            seq_ce_fwd=lambda: ops.seq_ce_fwd(logits, tok, True, PAD, 1),
            seq_ce_bwd=lambda: ops.seq_ce_bwd(one, logits, tok, lse, cnt, True, PAD, 1))
        own = {}
        for name, fn in calls.items():
            timed(fn, 3)
            own[name + "_call"] = summary([timed(fn, 4 * a.iters) for _ in range(a.reps)])
        rec = dict(what="nrtr_decoder_train_step", batch=N, tokens=T, length=L, layers=a.layers, d_model=C, d_inner=256,
                   dropout=p, reps=a.reps, iters=a.iters, torch=summary(times["torch"]), hip=summary(times["hip"]), **own,
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del dec, out_enc, qkv, dqkv, qp, dqp, kv, dkv, dout, logits
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
