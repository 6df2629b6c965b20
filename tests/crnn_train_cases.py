"""Cases shared by tests/test_crnn_train_host.py and tests/test_gpu_crnn_train.py (a helper module, not a test file): the CTC
case table and a float64 restatement of the arithmetic that tpspp_crnn_ctc_loss_fwd / _bwd implement
(include/tpspp_crnn_train.h), written from the header's formulas."""
import numpy as np
import torch
import torch.nn.functional as F

BLANK = 0


def text(s):
    """DICT36, lower-case: <BLK> = 0, '0'..'9' = 1..10, 'a'..'z' = 11..36."""
    return [1 + "0123456789abcdefghijklmnopqrstuvwxyz".index(ch) for ch in s.lower()]


# name -> (T, C, targets per image, input length per image (None: T))
CTC_CASES = {
    "T1": (1, 2, [[1]], None),
    "T2": (2, 3, [[1]], None),
    "hello": (9, 37, [text("hello")], None),                                   # an adjacent repeat: 5 + 1 <= 9
    "golden": (26, 37, [text("hello"), text("tps"), text("crnn2016")], None),
    "full": (26, 92, [list(range(1, 27))], None),                              # L = T without repeats: the one blank-free path
    "long": (40, 37, [[1 + j % 17 for j in range(35)]], None),                 # 71 states: more than one per lane; classes recur
    "empty": (5, 37, [[]], None),                                              # the blank path only
    "mixed": (12, 37, [text("hello"), [], text("aab"), text("z")], [12, 7, 4, 1]),   # "aab" in 4 positions: exactly feasible
}
INFEASIBLE = (text("aa"), 2)                                                   # needs 3 positions


def feasible(target, input_len):
    return len(target) + sum(a == b for a, b in zip(target, target[1:])) <= input_len


def ctc_case(name, extra=None):
    """-> (logits (N, T, C) float32, padded targets (N, Lmax) int32, target_len (N) int32, input_len (N) int32).
    extra: (target, input length) of one more image, put at position 1."""
    T, C, targets, input_len = CTC_CASES[name]
    targets = [list(t) for t in targets]
    input_len = [T] * len(targets) if input_len is None else list(input_len)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    logits = torch.randn((len(targets), T, C), generator=g) * 2.0
    if extra is not None:
        targets.insert(1, list(extra[0]))
        input_len.insert(1, extra[1])
        more = torch.randn((1, T, C), generator=torch.Generator().manual_seed(99)) * 2.0
        logits = torch.cat([logits[:1], more, logits[1:]])
    Lmax = max(len(t) for t in targets)
    padded = torch.zeros((len(targets), Lmax), dtype=torch.int32)
    for n, t in enumerate(targets):
        padded[n, :len(t)] = torch.tensor(t, dtype=torch.int32)
    return (logits, padded, torch.tensor([len(t) for t in targets], dtype=torch.int32),
            torch.tensor(input_len, dtype=torch.int32))


def ctc_torch(logits, padded, target_len, input_len, reduction="none", zero_infinity=False, blank=BLANK):
    """PyTorch's composition in the logits' dtype on their device -> the loss (its graph reaches `logits`)."""
    lp = F.log_softmax(logits, 2).permute(1, 0, 2)
    return F.ctc_loss(lp, padded.long().to(logits.device), input_len.long().to(logits.device),
                      target_len.long().to(logits.device), blank=blank, reduction=reduction, zero_infinity=zero_infinity)


def _lse(values):
    m = max(values)
    if m == -np.inf:
        return -np.inf
    return m + np.log(sum(np.exp(v - m) for v in values))


def ctc_formula64(logits, padded, target_len, input_len, blank=BLANK):
    """The header's formulas in float64 -> (loss (N), d sum(loss) / d logits (N, T, C)), rows t >= input_len zero."""
    x = logits.double().numpy()
    N, T, C = x.shape
    loss, grad = np.zeros(N), np.zeros((N, T, C))
    for n in range(N):
        L, Tn = int(target_len[n]), int(input_len[n])
        lab = [blank] * (2 * L + 1)
        lab[1::2] = [int(v) for v in padded[n, :L]]
        S = len(lab)
        lse = np.array([_lse(list(x[n, t])) for t in range(T)])
        lp = x[n] - lse[:, None]
        alpha = np.full((T, S), -np.inf)
        for t in range(Tn):
            for s in range(S):
                if t == 0:
                    alpha[t, s] = lp[t, lab[s]] if s < 2 else -np.inf
                    continue
                terms = [alpha[t - 1, s]]
                if s >= 1:
                    terms.append(alpha[t - 1, s - 1])
                if s >= 2 and lab[s] != blank and lab[s] != lab[s - 2]:
                    terms.append(alpha[t - 1, s - 2])
                alpha[t, s] = lp[t, lab[s]] + _lse(terms)
        if Tn == 0:
            loss[n] = 0.0 if L == 0 else np.inf
            continue
        loss[n] = -_lse([alpha[Tn - 1, S - 1]] + ([alpha[Tn - 1, S - 2]] if S >= 2 else []))
        if not np.isfinite(loss[n]):                                  # infeasible: the gradient is not defined
            continue
        beta = np.full((T, S), -np.inf)
        for t in range(Tn - 1, -1, -1):
            for s in range(S):
                if t == Tn - 1:
                    beta[t, s] = lp[t, lab[s]] if s >= S - 2 else -np.inf
                    continue
                terms = [beta[t + 1, s]]
                if s + 1 < S:
                    terms.append(beta[t + 1, s + 1])
                if s + 2 < S and lab[s + 2] != blank and lab[s + 2] != lab[s]:
                    terms.append(beta[t + 1, s + 2])
                beta[t, s] = lp[t, lab[s]] + _lse(terms)
            for c in range(C):
                states = [alpha[t, s] + beta[t, s] for s in range(S) if lab[s] == c]
                occ = np.exp(_lse(states) - lp[t, c] + loss[n]) if states else 0.0
                grad[n, t, c] = np.exp(lp[t, c]) - occ
    return torch.from_numpy(loss), torch.from_numpy(grad)
