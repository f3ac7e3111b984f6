/*
 * pgrc_oracle.c -- CPU restatement of PgRC's read-to-pseudogenome matching path.
 *
 * TEST INFRASTRUCTURE ONLY (see pgrc_oracle.h).  Written from the behavioural
 * specification of the reference; every
 * function cites the reference file:line it follows.  Pinned against the real
 * reference via oracle/_ref (tests/test_oracle_vs_ref.py) and the committed
 * golden fixtures (tests/golden/).
 */
#include "pgrc_oracle.h"

#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* ------------------------------------------------------------------ helpers */

/* utils/helper.cpp:263-276 (complementsLut); unknown symbols map to 0 there. */
static char complement_of(char c) {
    switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    case 'N': case 'n': return 'N';
    case 'U': case 'u': return 'A';
    case 'Y': case 'y': return 'R';
    case 'R': case 'r': return 'Y';
    case 'K': case 'k': return 'M';
    case 'M': case 'm': return 'K';
    case 'B': case 'b': return 'V';
    case 'D': case 'd': return 'H';
    case 'H': case 'h': return 'D';
    case 'V': case 'v': return 'B';
    default: return 0;
    }
}

/* utils/helper.cpp:383-393 */
void pgrc_or_revcomp(char *seq, uint64_t n) {
    uint64_t i = 0, j = n;
    while (i + 1 < j) {
        --j;
        char a = complement_of(seq[i]);
        seq[i] = complement_of(seq[j]);
        seq[j] = a;
        ++i;
    }
    if (i + 1 == j) seq[i] = complement_of(seq[i]);
}

/* utils/helper.cpp:277-283: val2sym "ACGTN" */
uint8_t pgrc_or_sym2val(char c) {
    switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    case 'N': return 4;
    default: return 0xFF;
    }
}

static int alphabet_order(const char *alphabet, char c) {
    const char *p = strchr(alphabet, c);
    return p ? (int)(p - alphabet) : -1;
}

static int symbols_per_byte(int sigma) {
    /* SymbolsPackingFacility::maxSymbolsPerElement (coders/SymbolsPackingFacility.cpp:125-130) */
    int spe = 0;
    unsigned long long v = 1;
    while (v * (unsigned)sigma - 1 <= 255) {
        v *= (unsigned)sigma;
        spe++;
    }
    return spe;
}

/* coders/SymbolsPackingFacility.cpp:143-178 (packSequence / packSuffixSymbols) */
void pgrc_or_pack_read(const char *read, uint32_t read_len, const char *alphabet, uint8_t *dst) {
    int sigma = (int)strlen(alphabet);
    int spe = symbols_per_byte(sigma);
    uint32_t i = 0, o = 0;
    while (i < read_len) {
        unsigned v = 0;
        for (int j = 0; j < spe; j++) {
            v *= (unsigned)sigma;
            if (i + (uint32_t)j < read_len) v += (unsigned)alphabet_order(alphabet, read[i + j]);
        }
        dst[o++] = (uint8_t)v;
        i += (uint32_t)spe;
    }
}

/* coders/SymbolsPackingFacility.cpp:216-236 (reverseSequence) */
void pgrc_or_unpack_read(const uint8_t *src, uint32_t read_len, const char *alphabet, char *dst) {
    int sigma = (int)strlen(alphabet);
    int spe = symbols_per_byte(sigma);
    for (uint32_t i = 0; i < read_len; i++) {
        unsigned v = src[i / (uint32_t)spe];
        int j = (int)(i % (uint32_t)spe);
        for (int k = spe - 1; k > j; k--) v /= (unsigned)sigma;
        dst[i] = alphabet[v % (unsigned)sigma];
    }
}

/* ---------------------------------------------------------- copMEM (mode c) */

static int isqrt_floor(int v) {
    int r = 0;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

/* matching/copmem/CopMEMMatcher.cpp:69-96, :111-137, ctor :571-577 */
int pgrc_or_copmem_derive(uint32_t seed_len, uint64_t pg_len, pgrc_or_copmem_params *out) {
    int L = (int)seed_len;
    int K;
    if (L > 110) K = 56;
    else if (L > 62) K = 44;
    else if (L > 53) K = 40;
    else if (L > 46) K = 36;
    else if (L > 42) K = 32;
    else if (L > 32) K = 28;
    else K = (L / 4 - 1) * 4;
    /* minMatchLength defaults to UINT32_MAX and is clipped to L (:574-575) */
    if (L < 24) return 1; /* "Minimal matching length too short" :77-80 */
    int kmml = (L / 4 - 1) * 4;
    if (kmml < K) K = kmml;
    int t = L - K + 1;
    if (t <= 0) return 2; /* "L and K mismatch" :115-118 */
    int k1, k2;
    if (t >= 20) {
        k1 = isqrt_floor(t) + 1;
        k2 = k1 - 1;
        if (k1 * k2 > t) { --k2; --k1; }
    } else if (t >= 15) { k1 = 5; k2 = 3; }
    else if (t >= 12) { k1 = 4; k2 = 3; }
    else if (t >= 10) { k1 = 5; k2 = 2; }
    else if (t >= 6) { k1 = 3; k2 = 2; }
    else { k1 = t; k2 = 1; }
    uint32_t hs;
    int i = 24;
    do {
        hs = ((uint32_t)1) << (i++);
    } while (i <= 31 && (uint64_t)hs < pg_len / (uint64_t)k1);
    out->L = L; out->K = K; out->k1 = k1; out->k2 = k2; out->hash_size = hs;
    return 0;
}

/* matching/copmem/Hashes.h:54-76 */
uint32_t pgrc_or_copmem_hash(int K, const char *str) {
    uint64_t h = (uint64_t)K;
    for (uint32_t j = 0; j < (uint32_t)K / 4; j++) {
        uint32_t w = (uint32_t)(uint8_t)str[4 * j] | ((uint32_t)(uint8_t)str[4 * j + 1] << 8) |
                     ((uint32_t)(uint8_t)str[4 * j + 2] << 16) |
                     ((uint32_t)(uint8_t)str[4 * j + 3] << 24);
        w &= (j < 3) ? 0x00FFFFFFu : 0x0000FFFFu;
        w += j;
        h ^= w;
        h *= 171717u;
    }
    return (uint32_t)h;
}

/* CopMEMMatcher.cpp:140-231, serial semantics (PgHelpers::numberOfThreads == 1):
 * every position p = 0, k1, 2*k1, ... <= G-K in ascending order; a bucket keeps
 * the first 13 positions and drops the rest (the reference's skippedList). */
int pgrc_or_index_build(const char *pg, uint64_t pg_len, uint32_t seed_len, pgrc_or_index *out) {
    memset(out, 0, sizeof *out);
    int e = pgrc_or_copmem_derive(seed_len, pg_len, &out->p);
    if (e) return e;
    out->pg_len = pg_len;
    const int K = out->p.K, k1 = out->p.k1;
    const uint32_t hs = out->p.hash_size, mask = hs - 1;
    uint32_t *cumm = (uint32_t *)calloc((size_t)hs + 2, sizeof(uint32_t));
    if (!cumm) return 3;
    uint64_t npos = (pg_len >= (uint64_t)K) ? (pg_len - (uint64_t)K) / (uint64_t)k1 + 1 : 0;
    /* pass 1: capped counts at cumm[h+1] */
    for (uint64_t i = 0; i < npos; i++) {
        uint32_t h = pgrc_or_copmem_hash(K, pg + i * (uint64_t)k1) & mask;
        if (cumm[h + 1] < PGRC_OR_BUCKET_CAP) cumm[h + 1]++;
    }
    /* exclusive prefix: cumm[h] = start of bucket h */
    uint64_t run = 0;
    for (uint64_t h = 0; h <= (uint64_t)hs; h++) {
        uint32_t c = cumm[h + 1];
        cumm[h + 1] = (uint32_t)run; /* temporarily: start of bucket h, stored at h+1 */
        run += c;
    }
    /* now cumm[h+1] = start(h); shift down so cumm[h] = start(h), keeping a fill cursor */
    uint32_t *cursor = (uint32_t *)malloc(((size_t)hs + 1) * sizeof(uint32_t));
    uint64_t *positions = (uint64_t *)malloc((size_t)(run + 2) * sizeof(uint64_t));
    if (!cursor || !positions) { free(cumm); free(cursor); free(positions); return 3; }
    for (uint64_t h = 0; h <= (uint64_t)hs; h++) cursor[h] = cumm[h + 1];
    for (uint64_t h = 0; h <= (uint64_t)hs; h++) cumm[h] = cursor[h];
    cumm[hs + 1] = (uint32_t)run;
    /* pass 2: fill in ascending p; a full bucket drops the position */
    for (uint64_t i = 0; i < npos; i++) {
        uint64_t p = i * (uint64_t)k1;
        uint32_t h = pgrc_or_copmem_hash(K, pg + p) & mask;
        if (cursor[h] < cumm[h + 1]) positions[cursor[h]++] = p;
    }
    free(cursor);
    out->cumm = cumm;
    out->positions = positions;
    out->count = run;
    return 0;
}

void pgrc_or_index_free(pgrc_or_index *idx) {
    free(idx->cumm);
    free(idx->positions);
    idx->cumm = NULL;
    idx->positions = NULL;
}

/* Test switch, off by default (= the reference's loops).  On: the per-read query stops as soon as the HIP kernel's
 * early-stop rule says that nothing can be accepted any more (pgrc_amd/csrc/copmem.hip, "Early stop"): a check of that
 * rule itself -- tests/test_early_stop_rule.py runs this restatement both ways and expects identical results. */
static int g_early_stop = 0;
static uint64_t g_probes = 0;
void pgrc_or_set_early_stop(int on) { g_early_stop = on; }
uint64_t pgrc_or_probe_count(int reset) {
    uint64_t v = __atomic_load_n(&g_probes, __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(&g_probes, 0, __ATOMIC_RELAXED);
    return v;
}

/* CopMEMMatcher.cpp:483-566 (processApproxMatchQueryTight).  The two extras serve the restatement of the HIP path's
 * schedule further down and are neutral otherwise: only_exact starts the query at limit 0, early applies the
 * early-stop rule, *by_rule reports that the rule (not the end of the seed list) ended the query. */
static uint64_t match_read_ex(const pgrc_or_index *idx, const char *pg, const char *read,
                              uint32_t read_len, uint8_t kmax, uint8_t kmin, uint8_t *cnt,
                              uint64_t *falses_out, uint64_t *cand_out, int only_exact, int early, int *by_rule) {
    const int K = idx->p.K, k2 = idx->p.k2;
    const uint32_t mask = idx->p.hash_size - 1;
    const uint64_t G = idx->pg_len;
    uint8_t limit = kmax;
    if (*cnt < kmax) limit = (uint8_t)(*cnt - 1); /* :488-489 */
    if (only_exact) limit = 0;
    if (by_rule) *by_rule = 0;
    const uint32_t head = (read_len / 8) * 8;      /* :495 */
    const uint64_t budget = (uint64_t)((read_len + 1 - (uint32_t)K) / (uint32_t)k2); /* :496-498 */
    uint64_t falses = 0, cands = 0;
    uint64_t best = PGRC_OR_NOT_MATCHED_POS;
    /* early-stop bookkeeping (only read when g_early_stop is set) */
    const uint32_t k1 = (uint32_t)idx->p.k1;
    const uint32_t rper = ((uint32_t)K + k1 * (uint32_t)k2 - 1) / (k1 * (uint32_t)k2) * k1;
    uint32_t rq = 0, rclean = 0, probes = 0;
    int rdirty = 0;
    for (uint32_t s = 0; s + (uint32_t)K < read_len + 1; s += (uint32_t)k2) { /* :503 */
        if (s) { /* the previous seed is done */
            if (rq == k1 - 1) { rclean += rdirty ? 0 : 1; rdirty = 0; }
            rq = (rq + 1 == rper) ? 0 : rq + 1;
            if (early && rclean > limit) {
                if (by_rule) *by_rule = 1;
                break;
            }
        }
        probes++;
        uint32_t h = pgrc_or_copmem_hash(K, read + s) & mask;
        uint32_t lo = idx->cumm[h], hi = idx->cumm[h + 1];
        if (lo == hi) continue;
        if (rq < k1 && (hi - lo >= PGRC_OR_BUCKET_CAP || (budget < falses && hi > lo + PGRC_OR_TRUNC_BUCKET))) rdirty = 1;
        if (budget < falses && hi > lo + PGRC_OR_TRUNC_BUCKET) hi = lo + PGRC_OR_TRUNC_BUCKET; /* :510-514 */
        for (uint32_t j = lo; j < hi; j++) {
            uint64_t sp = idx->positions[j];
            if ((uint64_t)s > sp) continue;                 /* :517-518 */
            if (sp - s + read_len > G) continue;            /* :519-520 */
            const char *t = pg + (sp - s);
            cands++;
            /* :523-539 -- 8-byte words with early exit; the outcome equals the
             * full head count compared with the limit (counts are monotone). */
            uint32_t m = 0;
            uint32_t i = 0;
            for (; i < head && m <= limit; i += 8)
                for (uint32_t b = 0; b < 8; b++) m += (read[i + b] != t[i + b]);
            if (m > limit) { falses++; continue; }
            /* :540-551 -- tail bytes; a reject here is counted twice */
            for (i = head; i < read_len; i++) m += (read[i] != t[i]);
            if (m > limit) { falses += 2; continue; }
            *cnt = (uint8_t)m;                              /* :552-555 */
            best = sp - s;
            if (m <= kmin) { /* :556-559 */
                if (falses_out) *falses_out += falses;
                if (cand_out) *cand_out += cands;
                __atomic_fetch_add(&g_probes, probes, __ATOMIC_RELAXED);
                return best;
            }
            limit = (uint8_t)(m - 1);                       /* :560 */
        }
    }
    if (falses_out) *falses_out += falses;
    if (cand_out) *cand_out += cands;
    __atomic_fetch_add(&g_probes, probes, __ATOMIC_RELAXED);
    return best;
}

uint64_t pgrc_or_copmem_match_read(const pgrc_or_index *idx, const char *pg, const char *read,
                                   uint32_t read_len, uint8_t kmax, uint8_t kmin, uint8_t *cnt,
                                   uint64_t *falses_out, uint64_t *cand_out) {
    return match_read_ex(idx, pg, read, read_len, kmax, kmin, cnt, falses_out, cand_out, 0, g_early_stop, NULL);
}

static void result_init(pgrc_or_result *res, uint64_t n, int with_counts) {
    for (uint64_t i = 0; i < n; i++) {
        res->pos[i] = PGRC_OR_NOT_MATCHED_POS;
        res->rc[i] = 0;
        res->mism[i] = PGRC_OR_NOT_MATCHED_CNT;
    }
    memset(res->hist, 0, sizeof res->hist);
    if (with_counts) res->hist[PGRC_OR_NOT_MATCHED_CNT] = n; /* ReadsMatchers.cpp:239 */
    res->matched = 0;
    memset(res->searched, 0, sizeof res->searched);
    memset(res->candidates, 0, sizeof res->candidates);
    memset(res->falses, 0, sizeof res->falses);
}

/* ReadsMatchers.cpp:162-172 (two passes) + :421-451 (CopMEMReadsApproxMatcher::executeMatching) */
int pgrc_or_match_copmem(const char *pg, uint64_t pg_len, const char *reads, uint64_t n,
                         uint32_t read_len, uint32_t seed_len, uint8_t kmax, uint8_t kmin,
                         int rev_compl_pg, int threads, int init, pgrc_or_result *res) {
    if (init) result_init(res, n, 1);
    char *rcpg = NULL;
    for (int pass = 0; pass < (rev_compl_pg ? 2 : 1); pass++) {
        const char *text = pg;
        if (pass == 1) {
            rcpg = (char *)malloc(pg_len + 1);
            if (!rcpg) return 3;
            memcpy(rcpg, pg, pg_len);
            rcpg[pg_len] = 0;
            pgrc_or_revcomp(rcpg, pg_len);
            text = rcpg;
        }
        pgrc_or_index idx;
        int e = pgrc_or_index_build(text, pg_len, seed_len, &idx);
        if (e) { free(rcpg); return e; }
        uint64_t searched = 0, cands = 0, falses = 0, matched = 0;
        uint64_t hist_delta_dec[256], hist_delta_inc[256];
        memset(hist_delta_dec, 0, sizeof hist_delta_dec);
        memset(hist_delta_inc, 0, sizeof hist_delta_inc);
#ifdef _OPENMP
        if (threads < 1) threads = 1;
#pragma omp parallel num_threads(threads)
#endif
        {
            uint64_t l_searched = 0, l_cands = 0, l_falses = 0, l_matched = 0;
            uint64_t l_dec[256], l_inc[256];
            memset(l_dec, 0, sizeof l_dec);
            memset(l_inc, 0, sizeof l_inc);
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1024)
#endif
            for (int64_t ii = 0; ii < (int64_t)n; ii++) {
                uint64_t i = (uint64_t)ii;
                if (res->mism[i] <= kmin) continue; /* :430 */
                l_searched++;
                uint8_t c = res->mism[i];
                uint64_t p = pgrc_or_copmem_match_read(&idx, text, reads + i * (uint64_t)read_len,
                                                       read_len, kmax, kmin, &c, &l_falses, &l_cands);
                if (p == PGRC_OR_NOT_MATCHED_POS) continue; /* :437-438 */
                if (c < res->mism[i]) {                      /* :439-447 */
                    if (res->mism[i] == PGRC_OR_NOT_MATCHED_CNT) l_matched++;
                    l_dec[res->mism[i]]++;
                    l_inc[c]++;
                    res->pos[i] = pass ? pg_len - (p + read_len) : p;
                    res->rc[i] = (uint8_t)pass;
                    res->mism[i] = c;
                }
            }
#ifdef _OPENMP
#pragma omp critical
#endif
            {
                searched += l_searched; cands += l_cands; falses += l_falses; matched += l_matched;
                for (int k = 0; k < 256; k++) { hist_delta_dec[k] += l_dec[k]; hist_delta_inc[k] += l_inc[k]; }
            }
        }
        for (int k = 0; k < 256; k++) res->hist[k] = res->hist[k] + hist_delta_inc[k] - hist_delta_dec[k];
        res->matched += matched;
        res->searched[pass] = searched;
        res->candidates[pass] = cands;
        res->falses[pass] = falses;
        pgrc_or_index_free(&idx);
    }
    free(rcpg);
    (void)threads;
    return 0;
}

/* ---- One query over BOTH strands at once (the HIP path's dual kernel), restated on the CPU: a test of that scheme, not
 * of the reference (tests/test_early_stop_rule.py expects pgrc_or_match_copmem_dual == pgrc_or_match_copmem).  kmin == 0.
 * Every seed probes the forward and the RC table (same hash); each strand is a query of its own whose limit is
 * additionally capped by what the other strand has found: forward by the RC count (a forward alignment only matters if
 * it is at least as good), RC by the forward count - 1 (it must be strictly better).  Each strand stops by the
 * early-stop rule against its capped limit.  Why this gives the reference's result: a query under ANY sequence of
 * limits that never falls below the smallest count m_min among its candidates accepts the FIRST candidate with m_min
 * (earlier accepted ones have larger counts, so the limit is still >= m_min when it comes) and nothing after it -- the
 * reference's final alignment; the caps never fall below the counts that still matter.  All of it presupposes that no
 * run cuts a bucket by the falses budget: U bounds the falses of any run over the candidates seen so far (1 for a
 * candidate whose head count alone exceeds the starting limit or that has no mismatch in the tail, else 2); U > budget when a
 * bucket of MORE THAN 4 entries is opened (the only thing the budget can change) -> the read is done again in the reference's
 * order (return 1). */
typedef struct { int limit; uint32_t cur; uint64_t best; uint64_t U; uint32_t rclean; int rdirty, active, found; } dual_side;

/* Speculative first attempt (round 4, the HIP kernel's a.spec): spec = small limit + 1 (0: none).  The query starts both
 * strands at min(L0, spec - 1) while U keeps bounding the falses of the run with the REAL starting limit L0; whatever it
 * finds is final, a read that finds nothing is queried again with spec = 0 (pgrc_or_match_copmem_dual below). */
static int g_dual_spec = 0;
void pgrc_or_set_dual_spec(int small_limit_plus_1) { g_dual_spec = small_limit_plus_1; }

static int dual_query(const pgrc_or_index *idx[2], const char *text[2], const char *read, uint32_t read_len,
                      uint8_t kmax, uint8_t cin, int spec, int *strand_out, uint64_t *pos_out, uint8_t *m_out, uint64_t cands[2]) {
    const int K = idx[0]->p.K, k2 = idx[0]->p.k2;
    const uint32_t k1 = (uint32_t)idx[0]->p.k1;
    const uint32_t mask = idx[0]->p.hash_size - 1;
    const uint64_t G = idx[0]->pg_len;
    const uint32_t head = (read_len / 8) * 8;
    const uint64_t budget = (uint64_t)((read_len + 1 - (uint32_t)K) / (uint32_t)k2);
    const int L0 = cin < kmax ? (int)cin - 1 : (int)kmax;
    const uint32_t rper = ((uint32_t)K + k1 * (uint32_t)k2 - 1) / (k1 * (uint32_t)k2) * k1;
    dual_side sd[2];
    const int Lstart = (spec && L0 >= spec) ? spec - 1 : L0;
    for (int x = 0; x < 2; x++) { sd[x].limit = Lstart; sd[x].cur = cin; sd[x].best = PGRC_OR_NOT_MATCHED_POS; sd[x].U = 0; sd[x].rclean = 0; sd[x].rdirty = 0; sd[x].active = 1; sd[x].found = 0; }
    uint32_t rq = 0, probes = 0;
#define DUAL_EFF(x) ((x) == 0 ? (sd[1].found && (int)sd[1].cur < sd[0].limit ? (int)sd[1].cur : sd[0].limit) \
                              : (sd[0].found && (int)sd[0].cur - 1 < sd[1].limit ? (int)sd[0].cur - 1 : sd[1].limit))
    for (uint32_t s = 0; s + (uint32_t)K < read_len + 1; s += (uint32_t)k2) {
        if (s) {
            for (int x = 0; x < 2; x++)
                if (rq == k1 - 1) { sd[x].rclean += sd[x].rdirty ? 0 : 1; sd[x].rdirty = 0; }
            rq = (rq + 1 == rper) ? 0 : rq + 1;
            for (int x = 0; x < 2; x++)
                if (sd[x].active && (int)sd[x].rclean > DUAL_EFF(x)) sd[x].active = 0;
        }
        if (!sd[0].active && !sd[1].active) break;
        const uint32_t h = pgrc_or_copmem_hash(K, read + s) & mask;
        int fwd_exact = 0;
        for (int x = 0; x < 2 && !fwd_exact; x++) {
            if (!sd[x].active) continue;
            probes++;
            const uint32_t lo = idx[x]->cumm[h], hi = idx[x]->cumm[h + 1];
            if (lo == hi) continue;
            /* the budget only ever CUTS a bucket to its first 4 entries (:510-514): while the buckets that are opened hold no
             * more than that, a run's falses count -- whatever it is -- changes nothing (round 4: k <= 50, where the
             * fingerprints reject nothing against the starting limit, sent 10.8 % of C3's reads back instead of 1.9 %) */
            if (sd[x].U > budget && hi - lo > PGRC_OR_TRUNC_BUCKET) { __atomic_fetch_add(&g_probes, probes, __ATOMIC_RELAXED); return 1; }
            if (rq < k1 && hi - lo >= PGRC_OR_BUCKET_CAP) sd[x].rdirty = 1;
            for (uint32_t j = lo; j < hi; j++) {
                const uint64_t sp = idx[x]->positions[j];
                if ((uint64_t)s > sp) continue;
                if (sp - s + read_len > G) continue;
                const char *t = text[x] + (sp - s);
                cands[x]++;
                uint32_t mh = 0, mt = 0;
                for (uint32_t i = 0; i < head; i++) mh += (read[i] != t[i]);
                for (uint32_t i = head; i < read_len; i++) mt += (read[i] != t[i]);
                sd[x].U += ((int)mh > L0 || mt == 0) ? 1 : 2;   /* no tail mismatch: head reject (1) or accepted (0), never 2 */
                const int m = (int)(mh + mt);
                if (m > DUAL_EFF(x)) continue;
                sd[x].cur = (uint32_t)m;
                sd[x].best = sp - s;
                sd[x].found = 1;
                sd[x].limit = m - 1;
                if (m == 0) {                      /* m <= kmin: this strand's query returns */
                    sd[x].active = 0;
                    if (x == 0) fwd_exact = 1;     /* ... and the RC pass would skip the read */
                    break;
                }
            }
        }
        if (fwd_exact) break;
    }
#undef DUAL_EFF
    __atomic_fetch_add(&g_probes, probes, __ATOMIC_RELAXED);
    if (sd[0].found && sd[0].cur == 0) { *strand_out = 0; *pos_out = sd[0].best; *m_out = 0; return 0; }
    if (sd[1].found && sd[1].cur < (sd[0].found ? sd[0].cur : (uint32_t)cin)) { *strand_out = 1; *pos_out = sd[1].best; *m_out = (uint8_t)sd[1].cur; return 0; }
    if (sd[0].found) { *strand_out = 0; *pos_out = sd[0].best; *m_out = (uint8_t)sd[0].cur; return 0; }
    *strand_out = -1;
    return 0;
}

int pgrc_or_match_copmem_dual(const char *pg, uint64_t pg_len, const char *reads, uint64_t n,
                              uint32_t read_len, uint32_t seed_len, uint8_t kmax, uint8_t kmin,
                              int threads, int init, pgrc_or_result *res, uint64_t *aborted_out) {
    if (kmin != 0) return 2;
    if (init) result_init(res, n, 1);
    if (threads < 1) threads = 1;
    char *rcpg = (char *)malloc(pg_len + 1);
    if (!rcpg) return 3;
    memcpy(rcpg, pg, pg_len);
    rcpg[pg_len] = 0;
    pgrc_or_revcomp(rcpg, pg_len);
    pgrc_or_index idxF, idxR;
    int e = pgrc_or_index_build(pg, pg_len, seed_len, &idxF);
    if (e) { free(rcpg); return e; }
    e = pgrc_or_index_build(rcpg, pg_len, seed_len, &idxR);
    if (e) { pgrc_or_index_free(&idxF); free(rcpg); return e; }
    const pgrc_or_index *idx[2] = {&idxF, &idxR};
    const char *text[2] = {pg, rcpg};
    uint64_t searched = 0, cands0 = 0, cands1 = 0, aborted = 0;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1024) num_threads(threads) reduction(+ : searched, cands0, cands1, aborted)
#endif
    for (int64_t ii = 0; ii < (int64_t)n; ii++) {
        const uint64_t i = (uint64_t)ii;
        if (res->mism[i] <= kmin) continue;
        searched++;
        const char *rd = reads + i * (uint64_t)read_len;
        int strand = -1;
        uint64_t pos = 0, cd[2] = {0, 0};
        uint8_t m = 0;
        int ab = dual_query(idx, text, rd, read_len, kmax, res->mism[i], g_dual_spec, &strand, &pos, &m, cd);
        if (!ab && strand < 0 && g_dual_spec)          /* the first attempt found nothing: the read again with its real limit */
            ab = dual_query(idx, text, rd, read_len, kmax, res->mism[i], 0, &strand, &pos, &m, cd);
        if (!ab) {
            cands0 += cd[0]; cands1 += cd[1];
            if (strand >= 0) { res->pos[i] = strand ? pg_len - (pos + read_len) : pos; res->rc[i] = (uint8_t)strand; res->mism[i] = m; }
            continue;
        }
        aborted++;
        cands0 += cd[0]; cands1 += cd[1];
        for (int pass = 0; pass < 2; pass++) {            /* the reference's order */
            if (res->mism[i] <= kmin) break;
            uint8_t c = res->mism[i];
            uint64_t f = 0, cdd = 0;
            const uint64_t p = match_read_ex(idx[pass], text[pass], rd, read_len, kmax, kmin, &c, &f, &cdd, 0, 1, NULL);
            if (pass) cands1 += cdd; else cands0 += cdd;
            if (p != PGRC_OR_NOT_MATCHED_POS && c < res->mism[i]) { res->pos[i] = pass ? pg_len - (p + read_len) : p; res->rc[i] = (uint8_t)pass; res->mism[i] = c; }
        }
    }
    memset(res->hist, 0, sizeof res->hist);
    res->matched = 0;
    for (uint64_t i = 0; i < n; i++) {
        res->hist[res->mism[i]]++;
        res->matched += res->mism[i] != PGRC_OR_NOT_MATCHED_CNT;
    }
    res->searched[0] = searched; res->searched[1] = 0;
    res->candidates[0] = cands0; res->candidates[1] = cands1;
    if (aborted_out) *aborted_out = aborted;
    free(rcpg);
    pgrc_or_index_free(&idxF);
    pgrc_or_index_free(&idxR);
    return 0;
}

/* ---- The HIP path's SCHEDULE for a two-pass run, restated on the CPU (a test of that schedule, not of the reference:
 * tests/test_early_stop_rule.py expects it to equal pgrc_or_match_copmem on every input).  With kmin == 0:
 *   K1  every read not yet matched exactly is screened on the RC text for an EXACT alignment (limit 0, early stop: one
 *       clean round); it is flagged if one is found and twice the false candidates seen stay within the falses budget
 *       (so no run of the real query, whose false counts are at most twice as high, could have cut a bucket before);
 *   K2  forward pass: a flagged read only looks for an exact forward alignment (which would win: the RC pass skips
 *       reads matched exactly).  Found within the budget -> final.  Proven absent by the early-stop rule -> the RC
 *       alignment of K1 is final (whatever the forward pass would have found is worse, and the RC pass would then reach
 *       that same first exact alignment).  Anything else -> the real forward query.  Unflagged reads: the real query;
 *   K3  the real RC pass over what is still not matched exactly. */
int pgrc_or_match_copmem_screened(const char *pg, uint64_t pg_len, const char *reads, uint64_t n,
                                  uint32_t read_len, uint32_t seed_len, uint8_t kmax, uint8_t kmin,
                                  int threads, int init, pgrc_or_result *res) {
    if (init) result_init(res, n, 1);
    if (threads < 1) threads = 1;
    char *rcpg = (char *)malloc(pg_len + 1);
    if (!rcpg) return 3;
    memcpy(rcpg, pg, pg_len);
    rcpg[pg_len] = 0;
    pgrc_or_revcomp(rcpg, pg_len);
    pgrc_or_index idxF, idxR;
    int e = pgrc_or_index_build(pg, pg_len, seed_len, &idxF);
    if (e) { free(rcpg); return e; }
    e = pgrc_or_index_build(rcpg, pg_len, seed_len, &idxR);
    if (e) { pgrc_or_index_free(&idxF); free(rcpg); return e; }
    const uint64_t budget = (uint64_t)((read_len + 1 - (uint32_t)idxF.p.K) / (uint32_t)idxF.p.k2);
    uint8_t *flag = (uint8_t *)calloc(n ? n : 1, 1);
    uint64_t *scr = (uint64_t *)malloc((n ? n : 1) * sizeof(uint64_t));
    const int screen = kmin == 0;
    uint64_t searched0 = 0, searched1 = 0, cands0 = 0, cands1 = 0;
    /* K1 */
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1024) num_threads(threads) reduction(+ : cands1)
#endif
    for (int64_t ii = 0; ii < (int64_t)n; ii++) {
        const uint64_t i = (uint64_t)ii;
        if (!screen || res->mism[i] <= kmin) continue;
        uint8_t c = res->mism[i];
        uint64_t f = 0, cd = 0;
        const uint64_t p = match_read_ex(&idxR, rcpg, reads + i * (uint64_t)read_len, read_len, kmax, kmin, &c, &f, &cd, 1, 1, NULL);
        cands1 += cd;
        if (p != PGRC_OR_NOT_MATCHED_POS && c == 0 && 2 * f <= budget) { flag[i] = 1; scr[i] = p; }
    }
    /* K2 */
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1024) num_threads(threads) reduction(+ : searched0, cands0)
#endif
    for (int64_t ii = 0; ii < (int64_t)n; ii++) {
        const uint64_t i = (uint64_t)ii;
        if (res->mism[i] <= kmin) continue;
        searched0++;
        const char *rd = reads + i * (uint64_t)read_len;
        if (flag[i]) {
            uint8_t c = res->mism[i];
            uint64_t f = 0, cd = 0;
            int by_rule = 0;
            const uint64_t p = match_read_ex(&idxF, pg, rd, read_len, kmax, kmin, &c, &f, &cd, 1, 1, &by_rule);
            cands0 += cd;
            if (p != PGRC_OR_NOT_MATCHED_POS && c == 0 && 2 * f <= budget) {
                res->pos[i] = p; res->rc[i] = 0; res->mism[i] = 0;
                continue;
            }
            if (p == PGRC_OR_NOT_MATCHED_POS && by_rule) {
                res->pos[i] = pg_len - (scr[i] + read_len); res->rc[i] = 1; res->mism[i] = 0;
                continue;
            }
        }
        uint8_t c = res->mism[i];
        uint64_t f = 0, cd = 0;
        const uint64_t p = match_read_ex(&idxF, pg, rd, read_len, kmax, kmin, &c, &f, &cd, 0, 1, NULL);
        cands0 += cd;
        if (p != PGRC_OR_NOT_MATCHED_POS && c < res->mism[i]) { res->pos[i] = p; res->rc[i] = 0; res->mism[i] = c; }
    }
    /* K3 */
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1024) num_threads(threads) reduction(+ : searched1, cands1)
#endif
    for (int64_t ii = 0; ii < (int64_t)n; ii++) {
        const uint64_t i = (uint64_t)ii;
        if (res->mism[i] <= kmin) continue;
        searched1++;
        uint8_t c = res->mism[i];
        uint64_t f = 0, cd = 0;
        const uint64_t p = match_read_ex(&idxR, rcpg, reads + i * (uint64_t)read_len, read_len, kmax, kmin, &c, &f, &cd, 0, 1, NULL);
        cands1 += cd;
        if (p != PGRC_OR_NOT_MATCHED_POS && c < res->mism[i]) { res->pos[i] = pg_len - (p + read_len); res->rc[i] = 1; res->mism[i] = c; }
    }
    memset(res->hist, 0, sizeof res->hist);
    res->matched = 0;
    for (uint64_t i = 0; i < n; i++) {
        res->hist[res->mism[i]]++;
        res->matched += res->mism[i] != PGRC_OR_NOT_MATCHED_CNT;
    }
    res->searched[0] = searched0; res->searched[1] = searched1;
    res->candidates[0] = cands0; res->candidates[1] = cands1;   /* [1] = K1 + K3 */
    free(flag); free(scr); free(rcpg);
    pgrc_or_index_free(&idxF);
    pgrc_or_index_free(&idxR);
    return 0;
}

/* ------------------------------------------- read-side seed index (d, i, e) */

/* ReadsMatchers.cpp:699-713 */
int pgrc_or_map_derive(uint32_t read_len, uint32_t seed_len, uint32_t min_chars_per_mismatch,
                       char mode, pgrc_or_map_params *out) {
    if (min_chars_per_mismatch == 0 || read_len == 0 || seed_len == 0) return 1;
    out->kmax = (uint8_t)(read_len / min_chars_per_mismatch);
    if (seed_len > read_len) seed_len = read_len;
    out->seed_len = seed_len;
    int upper = (mode >= 'A' && mode <= 'Z');
    out->kmin = upper ? out->kmax : 0;
    out->parts = (uint8_t)(read_len / seed_len);
    char lower = upper ? (char)(mode - 'A' + 'a') : mode;
    if (read_len == seed_len) out->matcher = (lower == 'c') ? 'c' : 'e'; /* :715-723 */
    else if (lower == 'd' || lower == 'i' || lower == 'c') out->matcher = lower;
    else return 2; /* "Unknown matching mode" :737-739 */
    return 0;
}

typedef struct {
    uint64_t hash;
    uint32_t idx;
} seed_ent;

static int seed_ent_cmp(const void *a, const void *b) {
    const seed_ent *x = (const seed_ent *)a, *y = (const seed_ent *)b;
    if (x->hash != y->hash) return x->hash < y->hash ? -1 : 1;
    /* equal keys iterate in reverse insertion order (libstdc++ unordered_multimap,
     * SURVEY.md Appendix C) => descending pattern index */
    if (x->idx != y->idx) return x->idx > y->idx ? -1 : 1;
    return 0;
}

static uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* Seed key.  The reference keys its multimap with CyclicHash<uint32> (rollinghash/cyclichash.h:100-123):
 * h = XOR_i rotl32(T[c_i], (n-1-i) mod 32) with a per-run random table T (characterhash.h:51-63), so the
 * VALUES are not reproducible -- but the EQUIVALENCE the hash induces is, and it is coarser than string
 * equality when n > 32: symbols at distance 32 share a rotation, so two seeds collide for every table iff,
 * per rotation class, every symbol occurs with the same parity (e.g. "A...C" ~ "C...A", "A...A" ~ "G...G"
 * across 32 positions).  Those candidates are real in the reference (they are verified and, in the approximate
 * modes, can be accepted), so the canonical key must reproduce exactly this equivalence: we evaluate the same
 * cyclic polynomial with two fixed, independent tables (64 key bits; non-equivalent seeds collide with
 * probability 2^-64, the reference's own accidental collisions with 2^-32 per comparison are not canonical). */
static uint32_t cyc_tab[2][256];
static int cyc_tab_ready = 0;
static void cyc_init(void) {
    if (cyc_tab_ready) return;
    for (int t = 0; t < 2; t++)
        for (int c = 0; c < 256; c++) {
            uint32_t x = (uint32_t)(mix64(0xC0FFEEull * (t + 1) + (uint64_t)c * 0x9E3779B97F4A7C15ull) >> 16);
            cyc_tab[t][c] = x;
        }
    /* A C G T N: the words of the HIP path (seedidx.hip, cyc_t0 / cyc_t1; there table(complement) = bit reversal of table(symbol),
     * which makes the key of a reverse complement a bijection of the key).  Beyond the canonical collisions there are table-dependent
     * ones on periodic runs (the XOR over the rotations of one residue class mod 1, 2 or 4 depends on sub-parities of the word): with
     * the same words both sides have the same ones, and the work counter `candidates` can be compared exactly. */
    {
        static const uint32_t w0[5] = {0x9E3779B9u, 0x7F4A7C15u, 0xA83E52FEu, 0x9D9EEC79u, 0x10824108u};
        static const uint32_t w1[5] = {0xBF58476Du, 0x1CE4E5B9u, 0x9DA72738u, 0xB6E21AFDu, 0x2545A2A4u};
        static const char sym[5] = {'A', 'C', 'G', 'T', 'N'};
        for (int k = 0; k < 5; k++) { cyc_tab[0][(uint8_t)sym[k]] = w0[k]; cyc_tab[1][(uint8_t)sym[k]] = w1[k]; }
    }
    cyc_tab_ready = 1;
}
static uint32_t rotl32(uint32_t x, uint32_t r) { r &= 31; return r ? (x << r) | (x >> (32 - r)) : x; }

/* eat() over m symbols at the given stride (cyclichash.h:119-122) */
static uint64_t cyc_hash_strided(const char *s, uint32_t m, uint32_t stride) {
    uint32_t h0 = 0, h1 = 0;
    for (uint32_t k = 0; k < m; k++) {
        uint8_t c = (uint8_t)s[(uint64_t)k * stride];
        h0 = rotl32(h0, 1) ^ cyc_tab[0][c];
        h1 = rotl32(h1, 1) ^ cyc_tab[1][c];
    }
    return ((uint64_t)h0 << 32) | h1;
}
/* update(out, in) (cyclichash.h:100-107): rotl1(h) ^ rotl(T[out], n mod 32) ^ T[in] */
static uint64_t cyc_roll(uint64_t h, uint32_t m, uint8_t out, uint8_t in) {
    uint32_t h0 = (uint32_t)(h >> 32), h1 = (uint32_t)h;
    h0 = rotl32(h0, 1) ^ rotl32(cyc_tab[0][out], m) ^ cyc_tab[0][in];
    h1 = rotl32(h1, 1) ^ rotl32(cyc_tab[1][out], m) ^ cyc_tab[1][in];
    return ((uint64_t)h0 << 32) | h1;
}

typedef struct {
    uint64_t key;
    uint32_t start, count;
} seed_slot;

int pgrc_or_match_seedindex(char mode, const char *pg, uint64_t pg_len, const char *reads,
                            uint64_t n, uint32_t read_len, uint32_t seed_len, uint8_t kmax,
                            uint8_t kmin, int rev_compl_pg, pgrc_or_result *res) {
    if (mode != 'e' && mode != 'd' && mode != 'i') return 2;
    if (seed_len > read_len) seed_len = read_len;
    const uint32_t P = (mode == 'e') ? 1 : read_len / seed_len; /* targetMismatches+1 */
    const uint32_t m = (mode == 'e') ? read_len : seed_len;     /* pattern length */
    const uint32_t stride = (mode == 'i') ? P : 1;
    const uint32_t span = (mode == 'i') ? m * P : m;            /* text window extent */
    result_init(res, n, mode != 'e');
    cyc_init();
    /* index every (read, part): ConstantLength...HashMatcher.cpp:23-42, :76-93 */
    uint64_t nent = n * P;
    seed_ent *ent = (seed_ent *)malloc((size_t)(nent ? nent : 1) * sizeof(seed_ent));
    if (!ent) return 3;
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t j = 0; j < P; j++) {
            const char *part = reads + i * read_len + ((mode == 'i') ? j : j * m);
            ent[i * P + j].hash = cyc_hash_strided(part, m, stride);
            ent[i * P + j].idx = (uint32_t)(i * P + j);
        }
    qsort(ent, (size_t)nent, sizeof(seed_ent), seed_ent_cmp);
    uint64_t tsize = 16;
    while (tsize < 2 * nent) tsize <<= 1;
    seed_slot *tab = (seed_slot *)calloc((size_t)tsize, sizeof(seed_slot));
    if (!tab) { free(ent); return 3; }
    for (uint64_t a = 0; a < nent;) {
        uint64_t b = a;
        while (b < nent && ent[b].hash == ent[a].hash) b++;
        uint64_t s = mix64(ent[a].hash) & (tsize - 1);
        while (tab[s].count) s = (s + 1) & (tsize - 1);
        tab[s].key = ent[a].hash; tab[s].start = (uint32_t)a; tab[s].count = (uint32_t)(b - a);
        a = b;
    }

    char *rcpg = NULL;
    for (int pass = 0; pass < (rev_compl_pg ? 2 : 1); pass++) {
        const char *text = pg;
        if (pass == 1) {
            rcpg = (char *)malloc(pg_len + 1);
            if (!rcpg) { free(ent); free(tab); return 3; }
            memcpy(rcpg, pg, pg_len);
            rcpg[pg_len] = 0;
            pgrc_or_revcomp(rcpg, pg_len);
            text = rcpg;
        }
        if (pg_len < span) continue;
        /* res->candidates[pass]: the (window, pattern) pairs with equal keys whose alignment lies inside the text -- the pairs the
         * reference looks at, whatever the read's state lets it do with them (a work counter: the HIP path reports the same) */
        uint64_t cands = 0;
        /* one rolling hash per residue class mod stride (ConstantLength...HashMatcher.h:105-137) */
        uint64_t *roll = (uint64_t *)malloc(sizeof(uint64_t) * stride);
        for (uint32_t r = 0; r < stride; r++)
            roll[r] = (r + (uint64_t)(m - 1) * stride < pg_len) ? cyc_hash_strided(text + r, m, stride) : 0;
        for (uint64_t t = 0; t + span <= pg_len; t++) {
            uint32_t r = (uint32_t)(t % stride);
            uint64_t key = roll[r];
            /* advance this residue's hash to window start t+stride */
            if (t + stride + (uint64_t)(m - 1) * stride < pg_len)
                roll[r] = cyc_roll(roll[r], m, (uint8_t)text[t], (uint8_t)text[t + (uint64_t)m * stride]);
            uint64_t s = mix64(key) & (tsize - 1);
            while (tab[s].count && tab[s].key != key) s = (s + 1) & (tsize - 1);
            if (!tab[s].count) continue;
            for (uint32_t a = tab[s].start; a < tab[s].start + tab[s].count; a++) {
                uint32_t pidx = ent[a].idx;
                uint64_t ri = pidx / P;
                uint32_t part = pidx % P;
                const char *rd = reads + ri * read_len;
                if (mode == 'e') { /* ReadsMatchers.cpp:203-224: a key hit must pass compareReadWithPattern == 0 */
                    cands++;
                    int eq = 1;
                    for (uint32_t k = 0; k < m && eq; k++) eq = rd[k] == text[t + k];
                    if (!eq) continue;
                    if (res->pos[ri] == PGRC_OR_NOT_MATCHED_POS) {
                        res->pos[ri] = pass ? pg_len - (t + read_len) : t;
                        if (pass) res->rc[ri] = 1;
                        res->mism[ri] = 0;
                        res->matched++;
                    }
                    continue;
                }
                /* ReadsMatchers.cpp:301-330 (d) / :368-397 (i) */
                uint64_t shift = (mode == 'i') ? part : (uint64_t)part * m;
                if (shift <= t && t - shift + read_len <= pg_len) cands++;
                if (res->mism[ri] <= kmin) continue;
                if (shift > t) continue;
                uint64_t p = t - shift;
                if (p + read_len > pg_len) continue;
                uint64_t stored = pass ? pg_len - (p + read_len) : p;
                if (res->pos[ri] == stored) continue;
                uint8_t limit = (res->mism[ri] == PGRC_OR_NOT_MATCHED_CNT) ? kmax : (uint8_t)(res->mism[ri] - 1);
                /* countSequenceMismatchesVsUnpacked, SymbolsPackingFacility.cpp:344-374 */
                uint32_t mm = 0;
                for (uint32_t k = 0; k < read_len && mm <= limit; k++) mm += (rd[k] != text[p + k]);
                uint8_t got = (mm > limit) ? PGRC_OR_NOT_MATCHED_CNT : (uint8_t)mm;
                if (got < res->mism[ri]) {
                    if (res->mism[ri] == PGRC_OR_NOT_MATCHED_CNT) res->matched++;
                    res->hist[res->mism[ri]]--;
                    res->hist[got]++;
                    res->pos[ri] = stored;
                    res->rc[ri] = (uint8_t)pass;
                    res->mism[ri] = got;
                }
            }
        }
        free(roll);
        res->candidates[pass] = cands;
    }
    if (mode == 'e') { /* DefaultReadsExactMatcher::transferMatchingResults :126-133 */
        res->hist[0] = res->matched;
        res->hist[PGRC_OR_NOT_MATCHED_CNT] = n - res->matched;
    }
    free(rcpg);
    free(ent);
    free(tab);
    return 0;
}

/* ---------------------------------------------------- mismatch extraction */

/* ReadsMatchers.cpp:40-66 + :548-559; code = (val(pg) << 4) + val(read), helper.cpp:358-362 */
void pgrc_or_extract_mismatches(const char *pg, uint64_t pos, const char *read, uint32_t read_len,
                                int rc, int reversed, uint8_t cnt, uint8_t *codes,
                                uint16_t *offsets) {
    char buf[256];
    memcpy(buf, read, read_len);
    if (rc) pgrc_or_revcomp(buf, read_len);
    const char *t = pg + pos;
    uint8_t c = 0;
    if (!reversed) {
        for (uint32_t i = 0; c < cnt && i < read_len; i++)
            if (buf[i] != t[i]) {
                codes[c] = (uint8_t)((pgrc_or_sym2val(t[i]) << 4) + pgrc_or_sym2val(buf[i]));
                offsets[c] = (uint16_t)i;
                c++;
            }
    } else {
        for (uint32_t i = read_len; c < cnt && i-- > 0;)
            if (buf[i] != t[i]) {
                codes[c] = (uint8_t)((pgrc_or_sym2val(complement_of(t[i])) << 4) +
                                     pgrc_or_sym2val(complement_of(buf[i])));
                offsets[c] = (uint16_t)(read_len - i - 1);
                c++;
            }
    }
}

/* ------------------------------------------------------ export of the matches */

/* One sink = the six ostringstreams SeparatedPseudoGenomeOutputBuilder::writeReadEntry appends to
 * (pseudogenome/persistence/SeparatedPseudoGenomePersistence.cpp:961-989). */
typedef struct {
    pgrc_or_export_streams *s;
    uint64_t last_written_pos;   /* lastWrittenPos (:962) */
    uint32_t L, width;
} ex_sink;

static void ex_put_len(uint8_t *dst, uint64_t at, uint32_t width, uint16_t v) {   /* writeReadLengthValue, helper.cpp:198-203 */
    if (width == 1) dst[at] = (uint8_t)v;
    else memcpy(dst + 2 * at, &v, 2);
}

static void ex_write_entry(ex_sink *k, uint64_t pos, uint16_t offset, uint32_t idx, int rev_comp, uint8_t cnt,
                           const uint8_t *codes, const uint16_t *offs) {
    pgrc_or_export_streams *s = k->s;
    k->last_written_pos = pos;                                                     /* :962 */
    ex_put_len(s->off, s->n_entries, k->width, offset);                             /* :966 */
    s->org_idx[s->n_entries] = idx;                                                 /* :967 */
    s->rev_comp[s->n_entries] = rev_comp ? 1 : 0;                                   /* :969 */
    s->mis_cnt[s->n_entries] = cnt;                                                 /* :971 */
    for (uint8_t i = 0; i < cnt; i++) s->mis_sym[s->n_mismatches + i] = codes[i];   /* :973-974 */
    uint8_t current = (uint8_t)(k->L - 1);                                          /* :976 */
    uint64_t at = s->n_mismatches;
    for (int i = (int)cnt - 1; i >= 0; i--) {                                       /* :977-981 */
        ex_put_len(s->mis_rev_off, at++, k->width, (uint16_t)(current - offs[i]));
        current = (uint8_t)(offs[i] - 1);
    }
    s->n_mismatches += cnt;
    s->n_entries++;                                                                 /* readsCounter, :988 */
}

/* updateEntry (ReadsMatchers.cpp:548-559) for read i at original index org */
static uint8_t ex_mismatches(const char *pg, const char *reads, uint32_t L, uint64_t i, uint64_t pos, int rc, uint8_t cnt,
                             uint32_t org, int pair_file, uint8_t *codes, uint16_t *offs) {
    const int reversed = pair_file ? (rc != (int)(org & 1u)) : rc;                  /* :553 */
    pgrc_or_extract_mismatches(pg, pos, reads + i * L, L, rc, reversed, cnt, codes, offs);
    return cnt;
}

/* DefaultReadsMatcher::exportMatchesInPgOrder (ReadsMatchers.cpp:563-595) after its sort: `order` lists the matched
 * reads by ascending position.  The reads list already on the pseudogenome is walked exactly like
 * writeReadsFromIterator does (:1004-1019), pause state and the -1 it returns once the list is exhausted included. */
int pgrc_or_export_pg_order(const char *pg, const char *reads, uint32_t L, const uint64_t *pos, const uint8_t *rc,
                            const uint8_t *mism, const uint32_t *order, uint64_t m, const uint32_t *read_org,
                            const uint8_t *list_off, const uint32_t *list_org, const uint8_t *list_rc, uint64_t h,
                            int pair_file, int byte_per_read_length, pgrc_or_export_streams *s) {
    ex_sink k = {s, 0, L, byte_per_read_length ? 1u : 2u};
    s->n_entries = s->n_mismatches = 0;
    s->off_width = k.width;
    /* iterator state: entry.pos / entry.offset of the list entry under the cursor (ExtendedReadsListWithConstantAccessOption::moveNext) */
    uint64_t it_pos = 0, cur = 0;
    uint16_t it_off = 0;
    int paused = 0, have = 0;                 /* have: the cursor stands on entry cur-1 */
    uint8_t codes[256];
    uint16_t offs[256];
    for (uint64_t j = 0; j <= m; j++) {
        const uint64_t stop = j < m ? pos[order[j]] : UINT64_MAX;                   /* the final writeReadsFromIterator() */
        uint64_t ret = UINT64_MAX;            /* what writeReadsFromIterator returns */
        int returned = 0;
        if (paused) {                                                               /* :1005-1010 */
            if (it_pos >= stop) { ret = k.last_written_pos; returned = 1; }
            else {
                ex_write_entry(&k, it_pos, it_off, list_org[cur - 1], list_rc ? list_rc[cur - 1] : 0, 0, codes, offs);
                paused = 0;
            }
        }
        while (!returned && cur < h) {                                              /* :1011-1017 */
            const uint64_t np = it_pos + list_off[cur];                             /* advanceEntryByOffset */
            it_off = (uint16_t)(np - it_pos);
            it_pos = np;
            cur++;
            have = 1;
            if (it_pos >= stop) { paused = 1; ret = k.last_written_pos; returned = 1; break; }
            ex_write_entry(&k, it_pos, it_off, list_org[cur - 1], list_rc ? list_rc[cur - 1] : 0, 0, codes, offs);
        }
        if (j == m) break;
        const uint64_t i = order[j];
        const uint64_t curr_pos = ret;                                              /* :579-580: entry(currPos), -1 once exhausted */
        const uint16_t offset = (uint16_t)(pos[i] - curr_pos);                      /* advanceEntryByPosition */
        const uint32_t org = read_org ? read_org[i] : (uint32_t)i;
        const uint8_t cnt = ex_mismatches(pg, reads, L, i, pos[i], rc[i], mism[i], org, pair_file, codes, offs);
        ex_write_entry(&k, pos[i], offset, org, rc[i], cnt, codes, offs);
        if (have) it_off = (uint16_t)(it_off - offset);                             /* writeExtraReadEntry, :991-997 */
    }
    s->last_pos = k.last_written_pos;
    return 0;
}

/* the per-entry part of exportMatchesInOriginalOrder (ReadsMatchers.cpp:655-667): every entry starts from a fresh
 * DefaultReadsListEntry(0); entry_read[k] == UINT32_MAX is a filler (position 0, no mismatches) */
int pgrc_or_export_entries(const char *pg, const char *reads, uint32_t L, const uint64_t *pos, const uint8_t *rc,
                           const uint8_t *mism, const uint32_t *entry_read, const uint32_t *entry_org, uint64_t ne,
                           int pair_file, int byte_per_read_length, pgrc_or_export_streams *s) {
    ex_sink k = {s, 0, L, byte_per_read_length ? 1u : 2u};
    s->n_entries = s->n_mismatches = 0;
    s->off_width = k.width;
    uint8_t codes[256];
    uint16_t offs[256];
    for (uint64_t e = 0; e < ne; e++) {
        const uint32_t i = entry_read[e];
        if (i == UINT32_MAX || mism[i] == PGRC_OR_NOT_MATCHED_CNT) {
            ex_write_entry(&k, 0, 0, entry_org[e], 0, 0, codes, offs);
            continue;
        }
        const uint8_t cnt = ex_mismatches(pg, reads, L, i, pos[i], rc[i], mism[i], entry_org[e], pair_file, codes, offs);
        ex_write_entry(&k, pos[i], (uint16_t)pos[i], entry_org[e], rc[i], cnt, codes, offs);
    }
    s->last_pos = k.last_written_pos;
    return 0;
}

/* ------------------------------------------------------ Pg-vs-Pg exact matches */

/* CopMEMMatcher::matchTexts -> processExactMatchQueryTight, matching/copmem/CopMEMMatcher.cpp:333-481, :604-622,
 * over the same serial seed index as the read matcher.  The destination text is scanned left to right in steps of
 * k2; the scan is SEQUENTIAL by nature (what a probe does depends on the last match found), and four 32-bit "side
 * context" registers l1/r1/l2/r2 are only refreshed when their 4 bytes lie inside the text, i.e. they keep a stale
 * value near the text ends (:381-382, :401-402).  All of that is restated here as it behaves. */
typedef struct {
    const pgrc_or_index *idx;
    const char *src, *dest;
    uint64_t N, N2;
    int dest_is_src, rev_compl;
    uint32_t min_len;
    int K, LK2, KLK24;
    uint32_t l1, l2, r1, r2;
    pgrc_or_text_match *out;
    uint64_t n_out, cap;
} mem_scan;

static uint32_t le32_at(const char *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

/* one probe of the destination at q; returns 1 when the scan must jump ahead (a match was pushed, or the window
 * lies inside the previous match on its diagonal) */
static int mem_visit(mem_scan *s, uint64_t q, int tail_loop) {
    const char *c2 = s->dest + q;
    const uint32_t h = pgrc_or_copmem_hash(s->K, c2) & (s->idx->p.hash_size - 1);
    const uint32_t lo = s->idx->cumm[h], hi = s->idx->cumm[h + 1];
    if (lo == hi) return 0;
    if (q >= (uint64_t)s->LK2) s->l2 = le32_at(c2 - s->LK2);                         /* :381 / :436 */
    if (q + (uint64_t)s->KLK24 + 4 <= s->N2) s->r2 = le32_at(c2 + s->KLK24);          /* :382 / :437 */
    for (uint32_t j = lo; j < hi; j++) {
        const uint64_t p = s->idx->positions[j];
        const char *c1 = s->src + p;
        if (s->dest_is_src && (s->rev_compl ? s->N2 - p < q : q >= p)) continue;      /* :389-392 */
        if (s->n_out) {                                                              /* :393-399 */
            const pgrc_or_text_match *b = &s->out[s->n_out - 1];
            if (q - p == b->pos_dest - b->pos_src && q + (uint64_t)s->K < b->pos_dest + b->length) return 1;
        }
        /* the tail loop reads these unconditionally (:456-457), which is out of bounds for the same positions;
         * treated like the main loop here (the value is unspecified in the reference) */
        (void)tail_loop;
        if (p >= (uint64_t)s->LK2) s->l1 = le32_at(c1 - s->LK2);                      /* :401 */
        if (p + (uint64_t)s->KLK24 + 4 <= s->N) s->r1 = le32_at(c1 + s->KLK24);       /* :402 */
        if (s->r1 != s->r2 && s->l1 != s->l2) continue;                              /* :404 */
        /* right extension: from the last symbol of the K-mer, pre-incrementing (:405-407) */
        uint64_t a = p + (uint64_t)s->K - 1, b2 = q + (uint64_t)s->K - 1;
        for (;;) {
            if (++a == s->N) break;
            if (++b2 == s->N2) break;
            if (s->src[a] != s->dest[b2]) break;
        }
        const uint64_t right = a;
        /* left extension: stops ON the first text symbol without stepping over it (:409-411) */
        uint64_t x = p, y = q;
        while (x != 0 && y != 0) {
            --x; --y;
            if (s->src[x] != s->dest[y]) break;
        }
        /* x, y now name the symbol BEFORE the match (or symbol 0, which is then left out of the match: the
         * reference's off-by-one at the text start) */
        if (right - x > (uint64_t)s->min_len && memcmp(c1, c2, (size_t)s->K) == 0) {   /* :413 */
            if (s->n_out == s->cap) {
                s->cap = s->cap ? 2 * s->cap : 1024;
                s->out = (pgrc_or_text_match *)realloc(s->out, s->cap * sizeof *s->out);
            }
            s->out[s->n_out].pos_src = x + 1;
            s->out[s->n_out].length = right - x - 1;
            s->out[s->n_out].pos_dest = y + 1;
            s->n_out++;
            return 1;
        }
    }
    return 0;
}

int pgrc_or_mem_match(const char *src, uint64_t N, const char *dest, uint64_t N2, int dest_is_src, int rev_compl,
                      uint32_t target_len, uint32_t min_match_len, pgrc_or_text_match **out, uint64_t *count) {
    pgrc_or_index idx;
    *out = NULL;
    *count = 0;
    int e = pgrc_or_index_build(src, N, target_len, &idx);
    if (e) return e;
    if ((int)min_match_len < idx.p.K) { pgrc_or_index_free(&idx); return 4; }         /* :606-609 */
    mem_scan s;
    memset(&s, 0, sizeof s);
    s.idx = &idx; s.src = src; s.dest = dest; s.N = N; s.N2 = N2;
    s.dest_is_src = dest_is_src; s.rev_compl = rev_compl; s.min_len = min_match_len;
    s.K = idx.p.K;
    s.LK2 = (idx.p.L - idx.p.K) / 2;                                                  /* :87-89 */
    s.KLK24 = idx.p.K + s.LK2 - 4;
    const uint64_t k2 = (uint64_t)idx.p.k2, block = 256 * k2;
    const uint64_t skip = (uint64_t)(idx.p.K / idx.p.k1 - 1);                         /* :352 */
    uint64_t i1 = 0;
    /* blocks of 256 probes: a jump ahead never leaves its block (:365-424) */
    for (; i1 + (uint64_t)s.K + block < N2 + 1; i1 += block)
        for (uint64_t i2 = 0; i2 < 256; i2++)
            if (mem_visit(&s, i1 + i2 * k2, 0)) i2 += skip;
    /* the remaining probes, one by one; here a jump carries through (:428-476) */
    for (; i1 + (uint64_t)s.K < N2 + 1; i1 += k2)
        if (mem_visit(&s, i1, 1)) i1 += skip * k2;
    pgrc_or_index_free(&idx);
    *out = s.out;
    *count = s.n_out;
    return 0;
}

void pgrc_or_mem_free(pgrc_or_text_match *m) { free(m); }

/* ------------------------------------------------------------------ row f3: the read sets */

#include <math.h>

/* qualityLut (utils/helper.cpp:284-327): 0 below '!', the probability 1 - 10^(-q/10) that a call of Phred quality q is
 * right for '!' + 0 .. '!' + 40, as a float; 1 for the next 59 characters.  (The reference writes the 41 values as
 * decimal literals; tests/test_divide_oracle.py compares this formula with the table of the compiled reference.) */
float pgrc_or_quality_lut(int c) {
    if (c < 33 || c > 132) return 0.f;
    if (c - 33 > 40) return 1.f;
    return (float)(1.0 - pow(10.0, -(double)(c - 33) / 10.0));
}

/* qualityScore2correctProbArithAvg(quality, 1, true) (utils/helper.cpp:452-475): fractionLength = rightLength = length, so
 * the left part is skipped and i starts at 0; val1 takes the even positions, val2 the odd ones, an odd last one val1 */
static double quality_arith_avg(const char *q, uint32_t len) {
    double val1 = 0, val2 = 0;
    uint32_t i = 0;
    for (; i < (len / 2) * 2; i += 2) {
        val1 += pgrc_or_quality_lut((unsigned char)q[i]);
        val2 += pgrc_or_quality_lut((unsigned char)q[i + 1]);
    }
    for (; i < len; i++) val1 += pgrc_or_quality_lut((unsigned char)q[i]);
    return (val1 + val2) / (int)len;
}

int pgrc_or_divide_reads(const char *reads, const char *quals, uint64_t n, uint32_t L, double error_limit, int simplified,
                         int separate_n, int n_reads_lq, uint8_t *hq_rows, uint8_t *lq_rows, uint8_t *n_rows,
                         uint32_t *lq_index, uint32_t *n_index, uint64_t counts[3], uint32_t symbols[3]) {
    /* the constructor, DividedPCLReadsSets.cpp:10-21 */
    const char *alpha_hq = (separate_n || n_reads_lq) ? "ACGT" : "ACGNT";
    const char *alpha_lq = separate_n ? "ACGT" : "ACGNT";
    const uint32_t rb_hq = (L + (strlen(alpha_hq) == 4 ? 4 : 3) - 1) / (strlen(alpha_hq) == 4 ? 4 : 3);
    const uint32_t rb_lq = (L + (strlen(alpha_lq) == 4 ? 4 : 3) - 1) / (strlen(alpha_lq) == 4 ? 4 : 3);
    const uint32_t rb_n = (L + 2) / 3;
    symbols[0] = (uint32_t)strlen(alpha_hq);
    symbols[1] = (uint32_t)strlen(alpha_lq);
    symbols[2] = separate_n ? 5u : 0u;
    counts[0] = counts[1] = counts[2] = 0;
    /* QualityDividingReadsSetIterator's constructor, DivisionReadsSetDecorators.cpp:14 */
    const int suffix_pos = (int)((double)L * (1 - error_limit));
    for (uint64_t i = 0; i < n; i++) {                       /* :68-87 */
        const char *r = reads + i * L;
        if (separate_n || n_reads_lq) {
            if (memchr(r, 'N', L)) {                         /* containsN, DivisionReadsSetDecorators.cpp:66-69 */
                if (separate_n) {
                    pgrc_or_pack_read(r, L, "ACGNT", n_rows + counts[2] * rb_n);
                    n_index[counts[2]++] = (uint32_t)i;
                } else {
                    pgrc_or_pack_read(r, L, alpha_lq, lq_rows + counts[1] * rb_lq);
                    lq_index[counts[1]++] = (uint32_t)i;
                }
                continue;
            }
        }
        int high = 1;
        if (error_limit < 1) {                               /* isQualityHigh, DivisionReadsSetDecorators.cpp:30-38 */
            const char *q = quals + i * L;
            /* quality[suffix_pos] of a std::string (signed chars); suffix_pos == L (error_limit 0) is its terminating 0 */
            if (simplified) high = suffix_pos < (int)L ? (signed char)q[suffix_pos] > '#' : 0;
            else high = (1 - quality_arith_avg(q, L) <= error_limit);
        }
        if (error_limit < 1 && !high) {
            pgrc_or_pack_read(r, L, alpha_lq, lq_rows + counts[1] * rb_lq);
            lq_index[counts[1]++] = (uint32_t)i;
        } else {
            pgrc_or_pack_read(r, L, alpha_hq, hq_rows + counts[0] * rb_hq);
            counts[0]++;
        }
    }
    return 0;
}

/* std::getline over a text in memory: the next line (without its newline) or 0 at the end; *len may be 0 for an empty line */
static int next_line(const char *t, uint64_t n, uint64_t *at, const char **line, uint64_t *len) {
    if (*at >= n) return 0;                                  /* nothing extracted at the end: the stream fails */
    const char *s = t + *at, *e = memchr(s, '\n', n - *at);
    *line = s;
    *len = e ? (uint64_t)(e - s) : n - *at;
    *at += *len + (e ? 1 : 0);
    return 1;
}

int64_t pgrc_or_fastq_records(const char *text, uint64_t bytes, const char *pair_text, uint64_t pair_bytes, int rev_compl_pair,
                              uint32_t L, char *reads, char *quals, uint64_t max_records) {
    uint64_t at[2] = {0, 0}, k = 0;
    const char *t[2] = {text, pair_text};
    const uint64_t n[2] = {bytes, pair_bytes};
    int pair = 0;                                            /* FASTQReadsSourceIterator::moveNext, ReadsSetIterator.cpp:206-224 */
    for (;; k++) {
        const int f = (pair && pair_text) ? 1 : 0;
        pair = !pair;
        const char *id, *line = "", *opt, *qual = "";
        uint64_t idl, linel = 0, optl, quall = 0;
        if (!next_line(t[f], n[f], &at[f], &id, &idl)) break;
        /* a cut-off last record: the reference goes on with whatever its strings held before (a getline on a stream at its
         * end leaves them alone) -- not restated, reported */
        if (!next_line(t[f], n[f], &at[f], &line, &linel) || !next_line(t[f], n[f], &at[f], &opt, &optl) ||
            !next_line(t[f], n[f], &at[f], &qual, &quall))
            return -3;
        uint64_t length = 0;
        while (length < linel && ((line[length] >= 'A' && line[length] <= 'Z') || (line[length] >= 'a' && line[length] <= 'z'))) length++;
        if (length != L) return -1;                          /* addRead: "Unsupported variable length reads" */
        if (k >= max_records) return -2;
        char *r = reads + k * L, *q = quals + k * L;
        memcpy(r, line, L);                                  /* getRead: line.resize(length) */
        for (uint32_t x = 0; x < L; x++) q[x] = x < quall ? qual[x] : 0;   /* getQualityInfo: quality.resize(length) */
        if (pair_text && rev_compl_pair && (k & 1)) pgrc_or_revcomp(r, L);  /* RevComplPairReadsSetIterator::getRead, :267-274 */
    }
    return (int64_t)k;
}
