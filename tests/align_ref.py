"""Plain numpy restatement of the word-timestamp path (csrc/align.hip, sonicscribe_amd/timestamps.py), checked itself by tests/test_align_host.py
and used as the reference of tests/test_gpu_align_kernel.py and tests/test_gpu_align.py.

  probs64        float64 softmax over the audio keys of scale * (q . k), per head                       (align_probs_kernel)
  normalise      (p - mean) / population std over the rows; std = 0 gives z = 0                          (align_reduce_kernel; Whisper divides by zero there)
  median_filter  width 7 along the audio axis with reflect padding; A <= 3 passes unchanged              (whisper/timing.py::median_filter)
  matrix         sum over heads of filtered z / H, heads in order
  dtw_f32        whisper/timing.py::dtw_cpu in fp32 with its tie rule, cell by cell, and the backtrace   (align_dtw_kernel: every cell is ONE fp32 add of a min, so
                 first_index    the audio index of the first path step of every text index                the wavefront order cannot change a bit)
  index_seconds / group_words: the host mapping and the word policy, restated without the package's code

The error bound of M (matrix_bound; DESIGN.md 6.9 derives it in the manner of 6.3 / 6.8), u = 2^-24, gamma_n = n u / (1 - n u):
  s      the inputs are element-type values, so every product q_i k_i is exact in fp32 (16 or 22 significant bits); 128 fused multiply-adds in sequence and the
         multiplication by the fp32 scale:  |s^ - s| <= D = gamma_130 scale sum_i |q_i k_i|
  p      the common shift of a softmax cancels, so its arguments are off by tau = max_a D + u max_a |s_a - max s| (the subtraction's rounding); expf is within
         1 ulp (relative 2u); the sum of A terms (thread-sequential, butterfly, 4 waves) has at most A additions on a path; one division:
         |p^ - p| <= rho p,  rho = exp(2 tau) (1 + u)^(A + 6) - 1
  mean   over L rows: |mu^ - mu| <= e_mu = max dp + gamma_(L+1) max p (1 + rho)
  d      p - mu, one subtraction: |d^ - d| <= e_d = max dp + e_mu + u max |d|
  std    the 2-norm is 1-Lipschitz and the L fused multiply-adds, the division and the root add gamma_(L+6) relatively: |sd^ - sd| <= e_sd = e_d + gamma_(L+6) (sd + e_d)
  z      d / sd, one division: |z^ - z| <= (e_d + |z| e_sd) / (sd - e_sd) + u (|z| + that)          - needs sd > e_sd: see THIN below
  median 1-Lipschitz in the sup norm over its window: the filtered value moves by at most the largest |z^ - z| of its 7 (reflected) columns
  M      H divisions and additions: the mean of the heads' bounds + gamma_(H+1) mean_h |z_f|
A column whose float64 std is exactly 0 (one row; one key) has z = 0 on both sides exactly - the kernel's mean of L equal values of 1.0, or of one value, is exact.
THIN: a column with 0 < std < 16 e_sd cannot be normalised to any accuracy by anybody (the division amplifies the softmax's error beyond bound); its probabilities
are compared BEFORE the normalisation only (|p^ - p| <= rho p + 2^-126), every M entry whose median window touches such a column is left out of the M comparison,
and THIN_CAP bounds the share of such columns so that a test cannot pass by declaring everything thin (tests/test_align_host.py checks the cap on the CPU for the
seeds the GPU test uses).
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
SCALE = F(1.0) / np.sqrt(F(128.0)).astype(F)      # the kernels' fp32 scale
THIN_FACTOR = 16.0
THIN_CAP = 0.02
FILTER = 7


def gamma(n):
    return n * U / (1.0 - n * U)


def probs64(q, k, scale=SCALE):
    """q [Tq][Hq][hd], k [Tk][Hkv][hd] (element-type values) -> (p [Hq][Tq][Tk] float64, s [Hq][Tq][Tk], absdot [Hq][Tq][Tk] = sum_i |q_i k_i|)"""
    q = np.asarray(q, np.float64); k = np.asarray(k, np.float64)
    Hq, Hkv = q.shape[1], k.shape[1]
    kk = np.repeat(k, Hq // Hkv, axis=1)                       # kv head of head h: h // (Hq / Hkv)
    s = np.einsum("nhd,ahd->hna", q, kk) * float(scale)
    absdot = np.einsum("nhd,ahd->hna", np.abs(q), np.abs(kk))
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True), s, absdot


def normalise(p, dtype=np.float64):
    """(p - mean) / std over axis -2 (the rows), population std; std = 0 -> 0"""
    p = np.asarray(p, dtype)
    mu = p.mean(axis=-2, keepdims=True)
    sd = np.sqrt(((p - mu) ** 2).mean(axis=-2, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0, (p - mu) / sd, 0.0)
    return z.astype(dtype)


def reflect_index(A, width=FILTER):
    """[A][width] source columns of the filter windows under numpy / torch 'reflect' padding (no edge repeat)"""
    pad = width // 2
    i = np.arange(A)[:, None] + np.arange(-pad, pad + 1)[None, :]
    i = np.where(i < 0, -i, i)
    return np.where(i >= A, 2 * (A - 1) - i, i)


def median_filter(z, width=FILTER):
    """median of `width` along the last axis with reflect padding; a last axis of <= width // 2 passes unchanged (whisper/timing.py::median_filter)"""
    z = np.asarray(z)
    A = z.shape[-1]
    if A <= width // 2:
        return z.copy()
    return np.sort(z[..., reflect_index(A, width)], axis=-1)[..., width // 2]


def matrix(p, dtype=np.float64):
    """p [H][L][A] -> M [L][A]: heads added in order, each as filtered z / H"""
    H = p.shape[0]
    M = np.zeros(p.shape[1:], dtype)
    for h in range(H):
        M = (M + (median_filter(normalise(p[h], dtype)) / dtype(H)).astype(dtype)).astype(dtype)
    return M


def dtw_f32(M):
    """whisper/timing.py::dtw_cpu on x = -M in fp32 -> (text indices, audio indices) of the path, in order.  Tie rule: c0 (diagonal) only if strictly below both
    others, else c1 (text step) only if strictly below both others, else c2 (audio step)."""
    x = (-np.asarray(M, F)).astype(F)
    N, A = x.shape
    cost = np.full((N + 1, A + 1), np.inf, F)
    trace = -np.ones((N + 1, A + 1), np.int8)
    cost[0, 0] = 0
    for j in range(1, A + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = F(x[i - 1, j - 1] + c)
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j, path = N, A, []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i -= 1; j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    path = np.array(path[::-1], np.int64).reshape(-1, 2)
    return path[:, 0], path[:, 1]


def first_index(text, audio, L):
    """t_n = the audio index of the first path step whose text index is n (Whisper's jump_times)"""
    t = np.full(L, -1, np.int32)
    for ti, ai in zip(text, audio):
        if 0 <= ti < L and t[ti] < 0:
            t[ti] = ai
    return t


def times_of(M):
    text, audio = dtw_f32(M)
    return first_index(text, audio, np.asarray(M).shape[0])


def matrix_bound(q, k, scale=SCALE):
    """q [Tq][Hq][hd], k [Tk][Hkv][hd] element-type values -> dict(M = float64 reference [Tq][Tk], bound = |M^ - M| bound [Tq][Tk], ok = entries held to it
    [Tq][Tk] bool, p = probabilities [Hq][Tq][Tk], p_bound, thin_share = share of (head, column) pairs that are thin) - the module docstring's derivation"""
    p, s, absdot = probs64(q, k, scale)
    H, L, A = p.shape
    D = gamma(130) * float(scale) * absdot
    tau = D.max(axis=-1, keepdims=True) + U * np.abs(s - s.max(axis=-1, keepdims=True)).max(axis=-1, keepdims=True)
    rho = np.exp(2 * tau) * (1 + U) ** (A + 6) - 1                     # [H][L][1]
    dp = rho * p
    mu = p.mean(axis=1, keepdims=True)
    d = p - mu
    sd = np.sqrt((d ** 2).mean(axis=1, keepdims=True))                 # [H][1][A]
    e_mu = dp.max(axis=1, keepdims=True) + gamma(L + 1) * (p * (1 + rho)).max(axis=1, keepdims=True)
    e_d = dp.max(axis=1, keepdims=True) + e_mu + U * np.abs(d).max(axis=1, keepdims=True)
    e_sd = e_d + gamma(L + 6) * (sd + e_d)
    exact0 = sd == 0
    thin = (~exact0) & (sd < THIN_FACTOR * e_sd)                        # [H][1][A]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(exact0, 0.0, d / sd)
        zb = (e_d + np.abs(z) * e_sd) / (sd - e_sd)
        zb = zb + U * (np.abs(z) + zb)
    zb = np.where(exact0, 0.0, np.where(thin, np.inf, zb))
    zb = np.broadcast_to(zb, p.shape)
    if A > FILTER // 2:
        win = reflect_index(A)
        zf = np.sort(z[..., win], axis=-1)[..., FILTER // 2]
        zfb = zb[..., win].max(axis=-1)
    else:
        zf, zfb = z, zb
    ok = np.isfinite(zfb).all(axis=0)
    M = np.zeros((L, A))
    for h in range(H):
        M = M + zf[h] / H
    with np.errstate(invalid="ignore"):
        bound = np.where(ok, np.where(np.isfinite(zfb), zfb, 0.0).mean(axis=0) + gamma(H + 1) * np.abs(zf).mean(axis=0), np.inf)
    return {"M": M, "bound": bound, "ok": ok, "p": p, "p_bound": dp + 2.0 ** -126, "thin_share": float(thin.mean())}


# ------------------------------------------------------------------------------------------ host mapping and word policy, restated
def index_seconds(idx, per_window_rows, chunk_seconds=30.0, step=0.08):
    """index into the audio-token run -> seconds: window w's rows follow those of the windows before it; its first row is w * chunk_seconds"""
    out = []
    for i in np.asarray(idx).reshape(-1):
        w, left = 0, int(i)
        while w + 1 < len(per_window_rows) and left >= per_window_rows[w]:
            left -= per_window_rows[w]; w += 1
        out.append(w * chunk_seconds + left * step)
    return np.array(out, np.float64)


def group_words(pieces):
    """pieces (text, ...) -> lists of piece indices: a word starts at a piece beginning with whitespace; a piece with a CJK / kana / hangul / Thai character stands alone"""
    def unspaced(t):
        return any(0x0E00 <= ord(c) <= 0x0E7F or 0x1100 <= ord(c) <= 0x11FF or 0x3040 <= ord(c) <= 0x30FF or 0x3130 <= ord(c) <= 0x318F or 0x31F0 <= ord(c) <= 0x31FF
                   or 0x2E80 <= ord(c) <= 0x2FDF or 0x3400 <= ord(c) <= 0x4DBF or 0x4E00 <= ord(c) <= 0x9FFF or 0xAC00 <= ord(c) <= 0xD7AF or 0xF900 <= ord(c) <= 0xFAFF
                   or 0x20000 <= ord(c) <= 0x2FA1F for c in t)
    words, alone = [], False
    for i, t in enumerate(pieces):
        own = unspaced(t)
        if not words or own or alone or t[:1].isspace():
            words.append([i])
        else:
            words[-1].append(i)
        alone = own
    return words


# ------------------------------------------------------------------------------------------ data of the GPU kernel test (shared with tests/test_align_host.py)
KERNEL_SHAPES = [  # (B, Tq, Tk, Hq, Hkv): every Tq in {1, 2, 17, 65}, every Tk in {1, 3, 4, 7, 16, 65, 375}, B in {1, 3}, both head shapes
    (1, 1, 1, 2, 1), (1, 2, 3, 2, 1), (3, 17, 4, 4, 2), (1, 65, 7, 2, 1), (3, 2, 16, 2, 1), (1, 17, 65, 4, 2), (3, 65, 375, 2, 1), (1, 1, 375, 4, 2),
    (1, 17, 1, 2, 1), (3, 65, 3, 4, 2), (1, 2, 65, 2, 1), (1, 65, 16, 4, 2),
]


SEED_SHIFT = {("bf16", (1, 2, 3, 2, 1)): 1}      # the cases whose first seed draws a thin column (two rows with nearly equal probabilities): the next seed


def kernel_data(shape, kind, seed=None):
    """q [B][Tq][Hq][128], k [B][Tk][Hkv][128] rounded to the element type.  q is scaled so that the scores spread over a few units (a softmax neither flat nor
    one-hot: columns with a healthy std)"""
    from attn_ref import rounder
    B, Tq, Tk, Hq, Hkv = shape
    if seed is None:
        seed = 20260128 + SEED_SHIFT.get((kind, tuple(shape)), 0)
    rng = np.random.default_rng([seed, B, Tq, Tk, Hq, Hkv, 0 if kind == "bf16" else 1])
    rt = rounder(kind)
    q = rt((2.0 * rng.standard_normal((B, Tq, Hq, 128))).astype(F))
    k = rt(rng.standard_normal((B, Tk, Hkv, 128)).astype(F))
    return q, k


def planted(Tq, Hq, Hkv, kind, seed=7):
    """a planted alignment: the keys come in Tq blocks of 4 .. 8 equal +-1 vectors (a plateau the median of 7 keeps, edges included), q_n = 3 x the vector of
    block n for every head, so row n's softmax sits on block n (score 34 against at most ~9 elsewhere).  f(n) = the first key of block n: a non-decreasing
    staircase, and the only cheapest path switches rows exactly there -> (q [1][Tq][Hq][128], k [1][Tk][Hkv][128], f [Tq])"""
    from attn_ref import rounder
    rng = np.random.default_rng([seed, Tq, Hq])
    rt = rounder(kind)
    lens = np.array([(4, 5, 8, 6)[n % 4] for n in range(Tq)])
    f = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    v = rng.choice([-1.0, 1.0], size=(Tq, Hkv, 128)).astype(F)
    k = np.repeat(v, lens, axis=0)[None]
    q = np.zeros((1, Tq, Hq, 128), F)
    for h in range(Hq):
        q[0, :, h] = 3.0 * v[:, h // (Hq // Hkv)]
    return rt(q), rt(k), f
