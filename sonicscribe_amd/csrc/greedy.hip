// The greedy controller: fused argmax over the lm_head's partial slabs + HF's greedy loop bookkeeping + the next step's embedding row and
// first RMSNorm, one block per row.  One kernel body, templated on the activation dtype T and eight flags - LP (per-token log-probabilities), GUARD (HF's logits
// processors), BIAS (per-request sequence bias), SAMPLE (temperature sampling), TOPK (the best alternatives of every step), GRAMMAR (a token automaton per
// request), TRUNC (top_k / top_p / min_p), LM (shallow fusion with an n-gram language model) - in the thirty-one combinations launch_greedy's table lists; and the prefill's kernel
// that writes a request's prompt ids into its history row for GUARD / BIAS.  Shares quant_emit_row (int8_util.h) with the decode-step consumers of elementwise.hip.
#include "common.h"
#include "kernels.h"

#include "int8_util.h"
#include "rowlp.h"
#include "truncsel.h"

// ---------------------------------------------------------------- argmax + greedy controller (generation/utils.py:2894-2936)
// LP (option token_logprobs): the block also returns log_softmax(l)[tok] of the token it emits.  Every thread keeps the sum lp_s of
// exp(r - lp_m) over the values it visits, lp_m being its running maximum `best`: one rescale per trip of the unrolled loop, then the trip's (up to
// 16) terms.  Threads are brought to their wave's maximum and added by the xor butterfly, waves to the block's maximum and added as a fixed tree by
// thread 0: one block, one order, whatever the grid.  exp is v_exp_f32 of the argument times log2(e); the closing log and subtraction are fp64.
// LP = false is the kernel as it was: everything below that belongs to the sum sits behind `if constexpr (LP)`.
// GUARD (sonic_set_generation): HF's repetition_penalty, no_repeat_ngram_size and suppress_tokens on the fp32 scores the argmax compares.
// The block first builds two vocabulary bitmaps in LDS from the row's history hist[b][0 .. kv_len[b]) (prompt ids, then every id emitted): "seen" (ids of
// the history) and "banned" (continuations of earlier occurrences of the last n - 1 ids, and the suppress list).  Integer ORs: no order in them.  The
// loop then reads the 4 bits of each map that belong to its f32x4 group: a seen score becomes s < 0 ? s * p : s / p (fp32 multiply, correctly rounded
// fp32 divide), a banned one -inf, in that order, behind the dump (raw logits) and ahead of the compare and the LP sum.  Thread 0 appends the emitted
// id at hist[b][kv_len[b]].  A row whose scores are all -inf emits token 0 (torch.argmax of equal values).  GUARD = false is the kernel as it was.
// BIAS (option request_bias; implies GUARD): HF's SequenceBiasLogitsProcessor, with NoBadWordsLogitsProcessor folded in as entries of bias -inf
// (generation/logits_process.py; the reference's hotwords, backend/asr.py:303-333, are what it serves), on the row's own table GreedyArgs.bias_tab.  Thread e of the
// prologue decides whether entry e applies to the history (L = 1: always; else L <= len and the last L - 1 ids equal its prefix) and leaves a flag in LDS; the first
// entry of every last-id group then adds the group's flagged biases to +0.0 in stored order - HF's order: the length-1 value, then the longer sequences in list
// order - and leaves (id, sum) in the LDS list and the id's bit in a third bitmap, "biased".  The loop reads that map's 4 bits with the others; a set bit scans the
// list (every lane reads the same word: a broadcast) and adds the sum, once, ahead of guard_score: the bias is HF's first processor.  An unset bit adds nothing
// (HF adds +0.0 there, which changes no compare and no exponential).  BIAS = false is the kernel as it was, GUARD or not.
// SAMPLE (option sampling; LP only): temperature sampling by the Gumbel-max identity.  Row b reads GreedyArgs.samp[3b ..]: the bits of its
// temperature t, its seed's low and high word.  t == 0: no division, no noise - the row's token and out_lp are the bits of the LP kernel.  t > 0: the compare runs
// on y_i = fdiv_rn(s_i, t) + g_i, s the fully processed score (bias, penalty, bans: HF's order, then TemperatureLogitsWarper), g_i = -ln(-ln(u_i)) Gumbel noise
// from Philox4x32-10 with key = the seed, counter = (i >> 2, n_new[b], 0, 0), word i & 3: one call per f32x4 group; u = ((word >> 9) + 0.5) * 2^-23 lies
// strictly inside (0, 1).  The first maximum of y is an exact draw from softmax(s / t); it depends on (scores, t, seed, step) alone - not on batch, row or
// slot.  The log-probability sum still runs over s, against its own running maximum (`rmax`; without SAMPLE that maximum is `best`), and out_lp is
// log_softmax(s)[tok] at temperature 1 - openai-whisper's convention, the one its fallback thresholds are calibrated on; the emitted token's s is recomputed
// from the slabs as the forced id's is.  Teacher forcing wins over sampling; step_logits stay raw.  The two logs are logf - v_log_f32 (1 ulp) times ln 2 in extended precision, a relative error
// of at most 1.5 * 2^-23 each: |g - exact| <= (1 + 16.64) * 1.5 * 2^-23 < 3.2e-6.
// TOPK (option top_logprobs = K, 1 .. 8; LP only): beside out_lp the block returns the K best ids of the step, ordered by (s descending, id
// ascending) over the ids with s > -inf, s the fully processed, unperturbed score the LP sum runs over, each with (float)(((double)s_k - (double)M) - log((double)lp_sum))
// - M and lp_sum the very values out_lp is formed from, so an emitted token that is among them carries out_lp's bits.  Every thread keeps the 8 best (value, id)
// pairs it has visited, sorted, in registers: a score is compared with the list's last value, and only a larger one is inserted (a thread visits its ids in
// ascending order, so among equal values the earlier id stays in front).  The lists are merged by K rounds of "butterfly argmax of the lanes' heads, the winner
// pops": per wave, then - the waves' lists in LDS, one per lane - by wave 1, while thread 0 of wave 0 does the step's bookkeeping.  The order is total (ids are
// unique), so the result does not depend on how the reduction is arranged.  Lanes 0 .. K - 1 of wave 1 write the record [lp | K alternative lps | K ids as fp32]
// at out_lp[(b * out_ld + n) * (1 + 2K)]; places beyond the finite scores hold (-inf, -1).  Forcing and sampling change the emitted token, never the
// alternatives; a finished row writes nothing.  TOPK = false is the kernel as it was: everything that belongs to the lists sits behind `if constexpr (TOPK)`.
// GRAMMAR (option grammar; LP and GUARD only): HF's PrefixConstrainedLogitsProcessor on a deterministic token automaton in CSR form that lives on
// the device (GreedyArgs.gram_ref[row]: [N | E | node_off[N + 1] | edge_tok[E] | edge_next[E]]; the edges of a node ascend by token id).  The row's state word
// gram_state[row] is -1 (free: the kernel as it was), n >= 0 (at node n) or -2 (it has left the grammar).  The prologue ORs the bits of the ids the row may emit -
// the edge tokens of n; the handle's EOS ids at -2 - into the zeroed "banned" map and inverts the map's words (the pad bits beyond V come out set: banned), two more
// barriers and one pass over the map; the n-gram and suppress bans then OR in as before.  Bans commute, so the fold gives the tokens of HF's chain SequenceBias ->
// RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> PrefixConstrained -> SuppressTokens; compare, LP sum, top-k lists and the Gumbel draw all run over the masked
// scores.  Thread 0 looks the emitted id - argmax, sample or forced id - up among the node's edges by binary search: found, the state is that edge's `next`; not
// found (a forced id outside the grammar, token 0 of a row whose allowed ids were all banned, any id at -2), it is -2.  A finished row changes nothing; no LDS is
// added.  GRAMMAR = false is the kernel as it was.
// TRUNC (option truncation; SAMPLE only): top_k / top_p / min_p on y = fdiv_rn(s, t), HF's warpers behind TemperatureLogitsWarper.  Row b reads
// GreedyArgs.trunc[3b ..]: top_k, the bits of top_p (0: off), the bits of lnm = float32(log(min_p)) (0: off; min_p = 1 is sent as -0.0).  A row with t = 0 or all
// three words 0 takes a block-uniform branch around everything below and runs the SAMPLE code.  Else the block finds the row's maximum of y, then the cut (kc, ic) -
// a key of y and an id - by the radix selects of truncsel.h, each pass recomputing y from the slabs (L2-resident) under the maps the prologue left in LDS; the loop's
// compare then admits an id only if trunc_keeps(key(y), id, kc, ic): the first maximum of y + g over the kept prefix.  The LP sum, out_lp, the alternatives and the
// dump see the untruncated scores.  With trunc_rec (test hook) one more pass counts the kept ids and finds the last of them in (y descending, id ascending):
// trunc_rec[3b ..] = the bits of its y, its id, n (an uncut row: 0, ~0, V).  TRUNC = false is the kernel as it was.
// LM (option lm; LP and GUARD only, never with GRAMMAR): shallow fusion.  GreedyArgs.lm_add[b][V] is the fp32 vector lm_step_kernel (lm.hip) built from the
// row's LM state right ahead of this launch; the loop reads it as f32x4 next to the slabs and forms r = rT(logit) + add[i] ahead of the request bias - the first
// processor of the chain, so bias, penalty, bans and temperature see the fused score, and so do the compare, the LP sum, out_lp, the alternatives and the truncation.
// The same add stands in the three places that form a score: the loop, y4 of the TRUNC twins, the recomputation of the emitted token's score.  The dump stays raw.
// Thread 0 leaves the emitted id - argmax, sample or forced id - in lm_tok[b] for the next lm_step_kernel; a finished row writes nothing.  No LDS is added.
// LM = false is the kernel as it was.
// The history's maps, the first-maximum butterfly, the sum's rescale, wave fold and block close, and the lists with their merges and record write live in
// rowlp.h: rows.hip (rows_kernel) shares them
extern __shared__ unsigned g_bits[];
__device__ __forceinline__ float bias_of(const int* ids, const float* sums, int n, int id) {
    float b = 0.f;
    for (int k = 0; k < n; ++k) if (ids[k] == id) b = sums[k];      // (ids are unique: one group per last id)
    return b;
}
// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between them
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// 23 bits, centred: every value is exact in fp32 and inside (0, 1).  logf is the library's: relatively accurate also at u next to 1, where -ln(u) is tiny (the
// hardware logarithm's 1 ulp is of ITS result): no 1 - u form needed
__device__ __forceinline__ float gumbel_of(unsigned word) {
    const float u = ((float)(word >> 9) + 0.5f) * 1.1920928955078125e-7f;
    return -logf(-logf(u));
}
#define LPB (SAMPLE ? rmax : best)      // what the LP sum is taken against: the running maximum of s
template <typename T, bool LP, bool GUARD = false, bool BIAS = false, bool SAMPLE = false, bool TOPK = false, bool GRAMMAR = false, bool TRUNC = false, bool LM = false>
__global__ __launch_bounds__(1024) void greedy_kernel(GreedyArgs a) {
    static_assert(!LM || (LP && GUARD && !GRAMMAR), "the language model lives in the log-probability guard instantiations without a grammar (one family per line of the table)");
    static_assert(SAMPLE || !TRUNC, "truncation lives in the sampling instantiations (it cuts what they draw from)");
    static_assert(!GRAMMAR || (LP && GUARD), "the grammar lives in the log-probability guard instantiations (it reuses their banned map)");
    static_assert(LP || !TOPK, "the alternatives live in the log-probability instantiations (they share their sum)");
    static_assert(GUARD || !BIAS, "the request bias lives in the guard instantiations (it needs their history)");
    static_assert(LP || !SAMPLE, "sampling lives in the log-probability instantiations (the fallback ladder reads them)");
    typedef typename ET<T>::v8 V8;
    __shared__ float sv[16];
    __shared__ int si[17];
    __shared__ int s_tok;
    __shared__ float ss_lp[LP ? (SAMPLE ? 32 : 16) : 1];
    [[maybe_unused]] float* const ss_m = ss_lp + (SAMPLE ? 16 : 0);      // SAMPLE: the waves' maxima of the unperturbed scores (sv holds those of y)
    __shared__ float s_tkv[TOPK ? 128 : 1];      // TOPK: the waves' lists, [place][wave] (lane w of wave 1 reads wave w's: consecutive words) ...
    __shared__ int s_tki[TOPK ? 128 : 1];        // ... and their ids
    __shared__ float s_tk_hand[TOPK ? 2 : 1];    // thread 0 -> wave 1: the block's maximum M and lp_sum, the values out_lp was formed from ...
    __shared__ int s_tk_col[1];                  // ... and the record's column n_new (-1: a finished row)
    __shared__ tr_u64 s_trh[TRUNC ? TRUNC_BINS : 1];      // TRUNC: the select's histogram ...
    __shared__ tr_u64 s_trw[TRUNC ? 16 : 1];              // ... the waves' totals of its scan (and the waves' maxima of y) ...
    __shared__ tr_u64 s_trr[TRUNC ? 4 : 1];               // ... and what a scan found
    [[maybe_unused]] float tv[8]; [[maybe_unused]] int ti[8]; [[maybe_unused]] float mv = -INFINITY; [[maybe_unused]] int mi = TK_NONE;
    if constexpr (TOPK) tk_init(tv, ti);
    float lp_m = -INFINITY, lp_s = 0.f;      // LP: the thread's sum is lp_s * exp(lp_m); a thread that saw nothing holds (-inf, 0)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* lg = a.logits + (long)b * a.V;
    [[maybe_unused]] const float* lm = nullptr;      // LM: the row's additive vector
    if constexpr (LM) lm = a.lm_add + (long)b * a.V;
    const long ks_stride = (long)a.mpad * a.V;
    float* dump = a.logits_dump ? a.logits_dump + (long)a.step_counter[b] * a.dump_stride_step + (long)b * a.V : nullptr;
    float best = -INFINITY; int bi = 0x7fffffff;
    // SAMPLE: the row's temperature, seed and step (block-uniform); rmax = the running maximum of s, which `best` (now over y) no longer is
    [[maybe_unused]] float temp = 0.f, rmax = -INFINITY; [[maybe_unused]] unsigned k0 = 0u, k1 = 0u, step_n = 0u; [[maybe_unused]] bool noisy = false;
    [[maybe_unused]] float* noise = nullptr;
    if constexpr (SAMPLE) {
        temp = __uint_as_float(a.samp[3 * b]); k0 = a.samp[3 * b + 1]; k1 = a.samp[3 * b + 2]; step_n = (unsigned)a.n_new[b];
        noisy = temp > 0.f;
        if (a.noise_out) noise = a.noise_out + (long)b * a.V;
    }
    // the first layer's norm weight for the tail of this kernel, requested before anything else (cold every step; behind the token's
    // embedding row it was one more dependent round trip)
    f32x4 gw0 = {0.f, 0.f, 0.f, 0.f}, gw1 = {0.f, 0.f, 0.f, 0.f};
    if (a.y && (a.d >> 3) <= 1024 && tid < (a.d >> 3)) { gw0 = *(const f32x4*)(a.norm_w + tid * 8); gw1 = *(const f32x4*)(a.norm_w + tid * 8 + 4); }
    [[maybe_unused]] unsigned* g_seen = nullptr; [[maybe_unused]] unsigned* g_ban = nullptr;
    [[maybe_unused]] unsigned* g_bia = nullptr; [[maybe_unused]] int* q_id = nullptr; [[maybe_unused]] float* q_sum = nullptr; [[maybe_unused]] int q_n = 0;
    [[maybe_unused]] int gst = -1, g_lo = 0, g_hi = 0; [[maybe_unused]] const int* g_tok = nullptr; [[maybe_unused]] const int* g_next = nullptr;      // GRAMMAR: the row's state and its node's edges
    if constexpr (GUARD) {
        const int nw = (a.V + 31) >> 5;
        g_seen = g_bits; g_ban = g_bits + nw;
        for (int w = tid; w < (BIAS ? 3 : 2) * nw; w += 1024) g_bits[w] = 0u;
        __syncthreads();
        if constexpr (GRAMMAR) {
            // the row's automaton; a state the blob does not hold (never staged by the engine) counts as "left"
            gst = a.gram_state[b];
            const int* gb = (const int*)a.gram_ref[b];
            if (gst >= 0 && (!gb || gst >= gb[0])) gst = -2;
            if (gst >= 0) { g_tok = gb + GRAM_HEAD + gb[0] + 1; g_next = g_tok + gb[1]; g_lo = max(gb[GRAM_HEAD + gst], 0); g_hi = min(gb[GRAM_HEAD + gst + 1], gb[1]); }
            if (gst != -1) {                      // block-uniform: the barriers below are reached by every thread or by none
                if (gst >= 0) for (int k = g_lo + tid; k < g_hi; k += 1024) guard_set(g_ban, g_tok[k], a.V);
                else if (tid < a.n_eos) guard_set(g_ban, a.eos[tid], a.V);
                __syncthreads();
                for (int w = tid; w < nw; w += 1024) g_ban[w] = ~g_ban[w];      // allowed -> banned; the pad bits beyond V are banned too
                __syncthreads();
            }
        }
        const int* h = a.hist + (long)b * a.hist_ld;
        const int len = min(max(a.kv_len[b], 0), a.hist_ld);
        if constexpr (BIAS) {
            // dynamic LDS behind the three maps: the group sums' ids [256], the sums [256], the entries' flags [256] (greedy_guard_lds)
            g_bia = g_bits + 2 * nw; q_id = (int*)(g_bits + 3 * nw); q_sum = (float*)(q_id + BIAS_MAX_ENTRIES);
            int* q_flag = q_id + 2 * BIAS_MAX_ENTRIES;
            const int* tab = a.bias_tab + 64 + (long)b * BIAS_ROW_WORDS;
            q_n = min(max(a.bias_tab[b], 0), BIAS_MAX_ENTRIES);
            const int* en = tab + tid * BIAS_ENTRY_WORDS;
            int last = -1;
            if (tid < q_n) {
                last = en[0];
                const int L = en[1];
                bool m = L >= 1 && L <= BIAS_MAX_LEN && L <= len;          // (L == len + 1 would fit its prefix; HF ignores it, so does this)
                if (m) { const int* tail = h + len - (L - 1); for (int k = 0; k < L - 1; ++k) m = m && tail[k] == en[3 + k]; }
                q_flag[tid] = (L == 1 || m) ? 1 : 0;                       // a single id has no prefix to match: it applies whatever the history holds
                q_id[tid] = -1;
            }
            __syncthreads();
            if (tid < q_n && (unsigned)last < (unsigned)a.V && (tid == 0 || en[-BIAS_ENTRY_WORDS] != last)) {      // the first entry of its last-id group
                float acc = 0.f; bool any = false;
                for (int k = tid; k < q_n && tab[k * BIAS_ENTRY_WORDS] == last; ++k)
                    if (q_flag[k]) { acc += __int_as_float(tab[k * BIAS_ENTRY_WORDS + 2]); any = true; }
                if (any) { q_id[tid] = last; q_sum[tid] = acc; guard_set(g_bia, last, a.V); }
            }
        }
        hist_maps(g_seen, g_ban, h, len, a.ngram, a.suppress, a.n_suppress, a.V, tid);
        __syncthreads();
    }
    [[maybe_unused]] unsigned kc = 0u; [[maybe_unused]] int ic = TRUNC_ID_ALL; [[maybe_unused]] bool cut = false;      // TRUNC: the row's cut; cut = false: every id is kept
    if constexpr (TRUNC) {
        const unsigned* tw = a.trunc + 3 * b;
        if (noisy && (tw[0] | tw[1] | tw[2]) != 0u) {      // block-uniform: the barriers below are reached by every thread or by none
            // the four y of group i: the loop's own arithmetic (slab sum in its order, rT, bias, guard_score, the correctly rounded quotient), without the noise
            auto y4 = [&](int i, float (&y)[4]) {
                f32x4 t = *(const f32x4*)(lg + i);
                for (int ks = 1; ks < a.ksplit; ++ks) t += *(const f32x4*)(lg + ks * ks_stride + i);
                [[maybe_unused]] unsigned sb = 0u, bb = 0u, qb = 0u;
                if constexpr (GUARD) { sb = g_seen[i >> 5] >> (i & 31); bb = g_ban[i >> 5] >> (i & 31); }
                if constexpr (BIAS) qb = (g_bia[i >> 5] >> (i & 31)) & 15u;
                [[maybe_unused]] f32x4 la = {0.f, 0.f, 0.f, 0.f};
                if constexpr (LM) la = *(const f32x4*)(lm + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float r = rT<T>(t[j]);
                    if constexpr (LM) r += la[j];
                    if constexpr (BIAS) if ((qb >> j) & 1u) r += bias_of(q_id, q_sum, q_n, i + j);
                    if constexpr (GUARD) r = guard_score(r, sb >> j, bb >> j, a.rep_penalty);
                    y[j] = __fdiv_rn(r, temp);
                }
            };
            float ym = -INFINITY;
            for (int i = tid * 4; i < a.V; i += 4096) {
                float y[4];
                y4(i, y);
#pragma unroll
                for (int j = 0; j < 4; ++j) ym = fmaxf(ym, y[j]);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ym = fmaxf(ym, __shfl_xor(ym, o, 64));
            float* const wmax = (float*)s_trw;
            if (lane == 0) wmax[wid] = ym;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < 16; ++w) ym = fmaxf(ym, wmax[w]);
            __syncthreads();                                   // (s_trw is the scans' from here on)
            if (ym > -INFINITY) {                              // (a row of -inf only keeps everything: token 0, as without the cut)
                trunc_cut(y4, a.V, tid, tw, ym, s_trh, s_trw, s_trr, kc, ic);
                cut = true;
                if (a.trunc_rec) {                             // the record: the kept ids counted, and the last of them - the lowest key, there the highest id
                    if (tid == 0) { s_trr[0] = 0ull; s_trr[1] = ~0ull; }
                    __syncthreads();
                    tr_u64 cnt = 0ull, low = ~0ull;
                    for (int i = tid * 4; i < a.V; i += 4096) {
                        float y[4];
                        y4(i, y);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const unsigned key = trunc_key(y[j]);
                            if (trunc_keeps(key, i + j, kc, ic)) { ++cnt; const tr_u64 v = ((tr_u64)key << 32) | (tr_u64)(0xffffffffu - (unsigned)(i + j)); low = v < low ? v : low; }
                        }
                    }
                    if (cnt) { atomicAdd(&s_trr[0], cnt); atomicMin(&s_trr[1], low); }
                    __syncthreads();
                    if (tid == 0) {
                        a.trunc_rec[3 * b] = __float_as_uint(trunc_unkey((unsigned)(s_trr[1] >> 32)));
                        a.trunc_rec[3 * b + 1] = 0xffffffffu - (unsigned)(s_trr[1] & 0xffffffffull);
                        a.trunc_rec[3 * b + 2] = (unsigned)s_trr[0];
                    }
                }
            }
        }
        if (!cut && a.trunc_rec && tid == 0) { a.trunc_rec[3 * b] = 0u; a.trunc_rec[3 * b + 1] = ~0u; a.trunc_rec[3 * b + 2] = (unsigned)a.V; }
    }
    // four strides per trip with all their slab loads issued first (the rolled form paid one L2 round trip per stride)
    constexpr int U = 4;
    for (int i0 = tid * 4; i0 < a.V; i0 += 1024 * 4 * U) {
        f32x4 v[U], w[U];
        [[maybe_unused]] f32x4 la[LM ? U : 1];      // LM: the groups of the row's vector, requested with the slabs
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 4096, ic = i < a.V ? i : 0;
            v[u] = *(const f32x4*)(lg + ic);
            w[u] = *(const f32x4*)(lg + (a.ksplit > 1 ? ks_stride : 0) + ic);
            if constexpr (LM) la[u] = *(const f32x4*)(lm + ic);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 4096;
            if (i >= a.V) break;
            f32x4 t = v[u];
            if (a.ksplit > 1) t += w[u];
            for (int ks = 2; ks < a.ksplit; ++ks) t += *(const f32x4*)(lg + ks * ks_stride + i);
            [[maybe_unused]] unsigned sb = 0u, bb = 0u;      // GUARD: the group's 4 bits of each map (i is a multiple of 4)
            if constexpr (GUARD) { sb = g_seen[i >> 5] >> (i & 31); bb = g_ban[i >> 5] >> (i & 31); }
            [[maybe_unused]] unsigned qb = 0u;               // BIAS: the group's 4 bits of the "biased" map
            if constexpr (BIAS) qb = (g_bia[i >> 5] >> (i & 31)) & 15u;
            [[maybe_unused]] float gz[4] = {0.f, 0.f, 0.f, 0.f};      // SAMPLE: the group's Gumbel values, one Philox call
            if constexpr (SAMPLE) if (noisy) {
                unsigned pw[4];
                philox4x32_10((unsigned)i >> 2, step_n, 0u, 0u, k0, k1, pw);
#pragma unroll
                for (int j = 0; j < 4; ++j) { gz[j] = gumbel_of(pw[j]); if (noise) noise[i + j] = gz[j]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float r = rT<T>(t[j]);              // logits are T in the reference, compared as fp32
                if (dump) dump[i + j] = r;
                if constexpr (LM) r += la[u][j];    // shallow fusion: the first processor, behind the dump (raw logits)
                if constexpr (BIAS) if ((qb >> j) & 1u) r += bias_of(q_id, q_sum, q_n, i + j);      // HF's order: the bias first, the penalty sees the biased score
                if constexpr (GUARD) r = guard_score(r, sb >> j, bb >> j, a.rep_penalty);
                if constexpr (TRUNC) {
                    const float q = noisy ? __fdiv_rn(r, temp) : r;
                    const float y = noisy ? q + gz[j] : r;
                    if (y > best && (!cut || trunc_keeps(trunc_key(q), i + j, kc, ic))) { best = y; bi = i + j; }      // the first maximum over the kept ids
                    rmax = fmaxf(rmax, r);
                } else if constexpr (SAMPLE) {
                    const float y = noisy ? __fdiv_rn(r, temp) + gz[j] : r;      // (-inf stays -inf: g is finite)
                    if (y > best) { best = y; bi = i + j; }
                    rmax = fmaxf(rmax, r);                                       // (t == 0: rmax == best, bit for bit)
                } else {
                    if (r > best) { best = r; bi = i + j; }   // strict > keeps the first maximum within a thread
                }
                if constexpr (TOPK) if (r > tv[7]) tk_insert(tv, ti, r, i + j);
                if constexpr (LP) v[u][j] = r;
            }
        }
        if constexpr (LP) {
            // the trip's values against the maximum so far (`best` covers them): the old sum is rescaled once (exp2(0) = 1 and s * 1 are exact when
            // the maximum did not move), then the terms are added in visiting order.  While nothing finite has been seen (the first trip, or trips
            // of -inf logits only) the sum stays 0: -inf - -inf is not formed, here or in the terms (exp(-inf - finite) = 0 is fine)
            lp_s = lp_rescale(lp_s, lp_m, LPB); lp_m = LPB;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (i0 + u * 4096 >= a.V) break;
#pragma unroll
                for (int j = 0; j < 4; ++j) lp_s += LPB > -INFINITY ? lp_exp(v[u][j] - LPB) : 0.f;
            }
        }
    }
    FIRST_MAX_WAVE(best, bi)
    if constexpr (SAMPLE) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, o, 64));
        if (lane == 0) ss_m[wid] = rmax;
    }
    if constexpr (LP) {
        lp_s = lp_wave_fold(lp_s, lp_m, LPB);      // every lane now holds the wave's maximum
        if (lane == 0) ss_lp[wid] = lp_s;
    }
    if constexpr (TOPK) tk_stage(tv, ti, a.topk, lane, wid, s_tkv, s_tki, mv, mi);
    if (lane == 0) { sv[wid] = best; si[wid] = bi; }
    __syncthreads();
    if constexpr (TOPK) if (wid == 1) tk_merge_waves(tv, ti, a.topk, lane, s_tkv, s_tki, mv, mi);      // beside thread 0's bookkeeping
    [[maybe_unused]] int tk_col = -1; [[maybe_unused]] float tk_m = 0.f, tk_sum = 0.f;
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
        float lp_sum = 0.f;
        if constexpr (LP) {
            if constexpr (SAMPLE) for (int w = 1; w < 16; ++w) rmax = fmaxf(rmax, ss_m[w]);
            lp_sum = lp_block_close(SAMPLE ? ss_m : sv, ss_lp, LPB);      // the waves' maxima of the scores the sum ran over
        }
        if constexpr (GUARD || SAMPLE) if (bi == 0x7fffffff) bi = 0;      // every score -inf: the first of equal values
        int tok = bi;
        const int fin = a.finished[b];
        bool running = false;
        if (fin) tok = a.pad_id;                 // finished rows emit the pad token (:2928-2929)
        else {
            if (a.force_ids) tok = a.force_ids[(long)b * a.force_ld + a.n_new[b]];   // teacher forcing (parity tests): feed this id instead
            a.out_ids[(long)b * a.out_ld + a.n_new[b]] = tok;
            if constexpr (LP) {
                float lt = LPB;                   // the emitted token's logit: the maximum, or under teacher forcing the forced id's value, summed
                // from the slabs in the main loop's order (v + w, then ks = 2 ...): the bits of the dumped logit.  SAMPLE: a sampled token is rarely the maximum of s
                if (SAMPLE ? (a.force_ids || noisy) && (unsigned)tok < (unsigned)a.V : a.force_ids != nullptr) {
                    float f = lg[tok];
                    if (a.ksplit > 1) f += lg[ks_stride + tok];
                    for (int ks = 2; ks < a.ksplit; ++ks) f += lg[ks * ks_stride + tok];
                    lt = rT<T>(f);
                    if constexpr (LM) lt += lm[tok];
                    if constexpr (BIAS) if ((g_bia[tok >> 5] >> (tok & 31)) & 1u) lt += bias_of(q_id, q_sum, q_n, tok);
                    if constexpr (GUARD) lt = guard_score(lt, g_seen[tok >> 5] >> (tok & 31), g_ban[tok >> 5] >> (tok & 31), a.rep_penalty);
                }
                a.out_lp[((long)b * a.out_ld + a.n_new[b]) * (TOPK ? 1 + 2 * a.topk : 1)] = (float)(((double)lt - (double)LPB) - log((double)lp_sum));
                if constexpr (TOPK) { tk_col = a.n_new[b]; tk_m = LPB; tk_sum = lp_sum; }
            }
            if constexpr (GUARD) { const int pos = a.kv_len[b]; if (pos >= 0 && pos < a.hist_ld) a.hist[(long)b * a.hist_ld + pos] = tok; }   // the token's position
            if constexpr (LM) a.lm_tok[b] = tok;         // the next lm_step_kernel consumes it
            if constexpr (GRAMMAR) if (gst != -1) {      // the transition: the emitted id among the node's ascending edge tokens, by bisection
                int ns = -2, lo = g_lo, hi = g_hi;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (g_tok[mid] < tok) lo = mid + 1; else hi = mid; }
                if (gst >= 0 && lo < g_hi && g_tok[lo] == tok) ns = g_next[lo];
                a.gram_state[b] = ns;
            }
            const int nn = a.n_new[b] + 1;
            a.n_new[b] = nn;
            bool stop = nn >= a.max_new[b];
            for (int e = 0; e < a.n_eos; ++e) stop |= (tok == a.eos[e]);
            if (stop) { a.finished[b] = 1; atomicSub(a.n_active, 1); } else running = true;
        }
        // device error word (SkinnyArgs.err = n_active[1]): a kernel of this step gave up on an in-kernel wait, its outputs are garbage.  The count of
        // running rows goes (and stays) far below zero: the loop stops at its next check and the host fails the batch (DEV_ERR_ACTIVE in engine_internal.h)
        if (a.dev_err && b == 0 && *a.dev_err) atomicMin(a.n_active, -(1 << 24));
        // Only a row that keeps running advances its context.  A finished row stays where it is (its later steps rewrite the same
        // cache slot and are discarded), so kv_len never exceeds prompt + max_new - 1 < max_ctx whatever the other rows' budgets are:
        // before, a [long prompt, small budget] row riding a [short prompt, large budget] batch walked past its cache region.
        if (running) {
            a.tok_pos[b] = a.kv_len[b];          // the new token sits right after the current context
            a.kv_len[b] += 1;
        }
        s_tok = tok;
        if (a.step_counter) a.step_counter[b] += 1;
    }
    if constexpr (TOPK) {
        // (words of their own: wave 1 may still be reading the waves' lists)
        if (tid == 0) { s_tk_hand[0] = tk_m; s_tk_hand[1] = tk_sum; s_tk_col[0] = tk_col; }
    }
    __syncthreads();
    if constexpr (TOPK) if (wid == 1 && lane < a.topk && s_tk_col[0] >= 0)
        tk_record(a.out_lp + ((long)b * a.out_ld + s_tk_col[0]) * (1 + 2 * a.topk), a.topk, lane, mv, mi, s_tk_hand[0], s_tk_hand[1]);
    const T* row = (const T*)a.table + (long)s_tok * a.d;
    T* xo = (T*)a.x;
    if (!a.y || (a.d >> 3) > 1024) {
        for (int c = tid; c < (a.d >> 3); c += 1024) *(V8*)(xo + (long)b * a.d + c * 8) = *(const V8*)(row + c * 8);
        return;
    }
    // next step's input row and, in the same pass, the first decoder layer's input RMSNorm of it (modeling_llama.py:60-65, :306):
    // one launch less per token step
    const int c = tid, nv = a.d >> 3;
    V8 xv;
    float ss = 0.f;
    if (c < nv) {
        xv = *(const V8*)(row + c * 8);
        *(V8*)(xo + (long)b * a.d + c * 8) = xv;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = (float)xv[j]; ss += f * f; }
    }
    ss = wave_sum(ss);
    __syncthreads();                         // sv is reused below
    if (lane == 0) sv[wid] = ss;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += sv[w];
    const float r = 1.0f / sqrtf(tot / a.d + a.norm_eps);
    float yo[8];
    if (c < nv) {
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { o[j] = (T)((j < 4 ? gw0[j & 3] : gw1[j & 3]) * rT<T>((float)xv[j] * r)); yo[j] = (float)o[j]; }
        *(V8*)((T*)a.y + (long)b * a.d + c * 8) = o;
    }
    if (a.qo.q) quant_emit_row(yo, c < nv, c, b, a.qo, sv, si);
}
#undef LPB

// a request's prompt ids into its history row (option generation guards): token t of the packed prompt plan is position tok_pos[t] of request
// tok_seq[t]; audio positions (src < 0) hold the placeholder id, as in HF's input_ids
__global__ void hist_prompt_kernel(const int* src, const int* tok_seq, const int* tok_pos, int n_tok, int audio_id, int* hist, int hist_ld) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tok) return;
    const int s = src[t], r = tok_seq[t], p = tok_pos[t];
    if (r >= 0 && r < 64 && p >= 0 && p < hist_ld) hist[(long)r * hist_ld + p] = s >= 0 ? s : audio_id;
}
void launch_hist_prompt(const int* src, const int* tok_seq, const int* tok_pos, int n_tok, int audio_id, int* hist, int hist_ld, hipStream_t s) {
    if (n_tok > 0) hipLaunchKernelGGL(hist_prompt_kernel, dim3((n_tok + 255) / 256), dim3(256), 0, s, src, tok_seq, tok_pos, n_tok, audio_id, hist, hist_ld);
}
// static LDS of the largest TRUNC instantiation (the TOPK twins; `; LDSByteSize` of the assembly): the histogram's 16 384 bytes, the scans' words, the lists' 1 300 and
// the reductions' - what the options' and the hook's 60 000-byte gate adds to the dynamic maps
size_t greedy_trunc_lds() { return 17848; }
static_assert(TRUNC_LDS_BYTES + 1464 == 17848, "greedy_trunc_lds: the histogram is part of the figure");
size_t greedy_guard_lds(int V, bool bias) { return (size_t)(bias ? 3 : 2) * ((V + 31) / 32) * 4 + (bias ? (size_t)3 * BIAS_MAX_ENTRIES * 4 : 0); }
// One family of the table below: its grid, block and LDS request, for fp32 rows (SONIC_MODE_F32: fp32 logits, table and rows) and for the 16-bit kinds
template <bool LP, bool GUARD, bool BIAS, bool SAMPLE, bool TOPK = false, bool GRAMMAR = false, bool TRUNC = false, bool LM = false>
static void greedy_launch(const GreedyArgs& a, hipStream_t s) {
    if constexpr (SAMPLE && !TRUNC) if (a.trunc) return greedy_launch<LP, GUARD, BIAS, SAMPLE, TOPK, GRAMMAR, true, LM>(a, s);      // trunc (counts only together with samp) = option truncation: the family's TRUNC twin
    const size_t lds = GUARD ? greedy_guard_lds(a.V, BIAS) : 0;      // GUARD: two vocabulary bitmaps of dynamic LDS; BIAS: a third and the matched list; GRAMMAR: nothing more
    if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, LP, GUARD, BIAS, SAMPLE, TOPK, GRAMMAR, TRUNC, LM>), dim3(a.B), dim3(1024), lds, s, a); return; }
    DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, LP, GUARD, BIAS, SAMPLE, TOPK, GRAMMAR, TRUNC, LM>), dim3(a.B), dim3(1024), lds, s, a));
}
// The thirty-one families, chosen from the arguments: out_lp = option token_logprobs, hist = generation guards, bias_tab (counts only together with hist) = request
// bias, samp (counts only together with out_lp) = option sampling, topk in 1 .. 8 (counts only together with out_lp) = option top_logprobs, gram_state with gram_ref
// (counts only together with out_lp and hist) = option grammar, lm_add with lm_tok (likewise; never beside a grammar) = option lm.  One line per family: a combination that is not listed is not instantiated.
void launch_greedy(const GreedyArgs& a, hipStream_t s) {
    const bool lp = a.out_lp != nullptr, guard = a.hist != nullptr, bias = guard && a.bias_tab, sample = lp && a.samp, topk = lp && a.topk >= 1 && a.topk <= 8;
    const bool gram = lp && guard && a.gram_state && a.gram_ref;
    if (gram) {
        //                                        LP     GUARD  BIAS   SAMPLE TOPK   GRAMMAR
        if (topk && sample && bias)  return greedy_launch<true,  true,  true,  true,  true,  true >(a, s);
        if (topk && sample)          return greedy_launch<true,  true,  false, true,  true,  true >(a, s);
        if (topk && bias)            return greedy_launch<true,  true,  true,  false, true,  true >(a, s);
        if (topk)                    return greedy_launch<true,  true,  false, false, true,  true >(a, s);
        if (sample && bias)          return greedy_launch<true,  true,  true,  true,  false, true >(a, s);
        if (sample)                  return greedy_launch<true,  true,  false, true,  false, true >(a, s);
        if (bias)                    return greedy_launch<true,  true,  true,  false, false, true >(a, s);
        return greedy_launch<true,  true,  false, false, false, true >(a, s);
    }
    if (lp && guard && a.lm_add && a.lm_tok) {
        //                                        LP     GUARD  BIAS   SAMPLE TOPK   GRAMMAR TRUNC LM
        if (topk && sample && bias)  return greedy_launch<true,  true,  true,  true,  true,  false, false, true >(a, s);
        if (topk && sample)          return greedy_launch<true,  true,  false, true,  true,  false, false, true >(a, s);
        if (topk && bias)            return greedy_launch<true,  true,  true,  false, true,  false, false, true >(a, s);
        if (topk)                    return greedy_launch<true,  true,  false, false, true,  false, false, true >(a, s);
        if (sample && bias)          return greedy_launch<true,  true,  true,  true,  false, false, false, true >(a, s);
        if (sample)                  return greedy_launch<true,  true,  false, true,  false, false, false, true >(a, s);
        if (bias)                    return greedy_launch<true,  true,  true,  false, false, false, false, true >(a, s);
        return greedy_launch<true,  true,  false, false, false, false, false, true >(a, s);
    }
    //                                        LP     GUARD  BIAS   SAMPLE TOPK
    if (topk && sample && bias)  return greedy_launch<true,  true,  true,  true,  true >(a, s);
    if (topk && sample && guard) return greedy_launch<true,  true,  false, true,  true >(a, s);
    if (topk && sample)          return greedy_launch<true,  false, false, true,  true >(a, s);
    if (topk && bias)            return greedy_launch<true,  true,  true,  false, true >(a, s);
    if (topk && guard)           return greedy_launch<true,  true,  false, false, true >(a, s);
    if (topk)                    return greedy_launch<true,  false, false, false, true >(a, s);
    //                                LP     GUARD  BIAS   SAMPLE
    if (sample && bias)  return greedy_launch<true,  true,  true,  true >(a, s);
    if (sample && guard) return greedy_launch<true,  true,  false, true >(a, s);
    if (sample)          return greedy_launch<true,  false, false, true >(a, s);
    if (bias && lp)      return greedy_launch<true,  true,  true,  false>(a, s);
    if (bias)            return greedy_launch<false, true,  true,  false>(a, s);
    if (guard && lp)     return greedy_launch<true,  true,  false, false>(a, s);
    if (guard)           return greedy_launch<false, true,  false, false>(a, s);
    if (lp)              return greedy_launch<true,  false, false, false>(a, s);
    return greedy_launch<false, false, false, false>(a, s);
}
