/* The stall of one key's WGL search (a CPU analysis tool, not product code):
 * the canonical WGL DFS of oracle/jh_oracle.c, as wgl_shape.c's wgl_at runs
 * it, recording the stall -- the inserts since the deepest layer last rose --
 * that phase 2's sequential search publishes for the late helpers (round 7).
 * Built and driven by tools/shape/stall_study.py. */
#include "../../oracle/jh_oracle.c"

/* thr[0..n_thr): stall thresholds, ascending. out: [0] total inserts (capped
 * by budget), [1] verdict, [2] n_ok, [3] the largest stall; first[i]: the
 * insert count at which the stall first reached thr[i] (-1: never). */
int wgl_stall(const jh_history *h, const int64_t *sel, int64_t m, int64_t init, int64_t budget,
              const int64_t *thr, int n_thr, int64_t *first, int64_t *out) {
    orc_key kk; orc_key_prepare(h, sel, m, &kk); const orc_key *k = &kk;
    out[0] = out[3] = 0; out[1] = -1; out[2] = k->n_ok;
    for (int i = 0; i < n_thr; i++) first[i] = -1;
    if (k->status || k->n_ok == 0) { orc_key_free(&kk); return -1; }
    cset memo; cset_init(&memo);
    int64_t scap = 256, depth = 0;
    frame *st = (frame *)malloc(sizeof(frame) * scap);
    uint32_t t = 0, tmax = 0; int64_t s = init; int start = 0;
    int64_t last_rise = 0, stall_max = 0;
    int next = 0;             /* the first threshold not reached yet */
    uint64_t mask[MW] = {0};
    int verdict = -1;
    for (;;) {
        const int32_t *W = k->w_ops + k->w_off[t];
        int w = k->w_off[t + 1] - k->w_off[t];
        int took = 0;
        for (int i = start; i < w; i++) {
            if (bit_get(mask, i)) continue;
            const orc_op *o = &k->ops[W[i]];
            int64_t s2;
            if (!cas_step(o->f, o->v1, o->v2, s, &s2)) continue;
            cfg c; c.s = s2;
            cfg_lift(k, t, mask, i, &c.t, c.m);
            if (cset_has(&memo, &c)) continue;
            if (memo.n >= budget) { verdict = JH_UNKNOWN; goto done; }
            cset_add(&memo, &c);
            if (depth == scap) { scap *= 2; st = (frame *)realloc(st, sizeof(frame) * scap); }
            st[depth].t = t; st[depth].i = i; st[depth].s = s; memcpy(st[depth].m, mask, sizeof mask); depth++;
            t = c.t; s = c.s; memcpy(mask, c.m, sizeof mask); start = 0;
            if (t > tmax) { tmax = t; last_rise = memo.n; }
            {
                const int64_t stall = memo.n - last_rise;
                if (stall > stall_max) stall_max = stall;
                while (next < n_thr && stall_max >= thr[next]) first[next++] = memo.n;
            }
            if (t == (uint32_t)k->n_ok) { verdict = JH_VALID; goto done; }
            took = 1;
            break;
        }
        if (took) continue;
        if (depth == 0) { verdict = JH_INVALID; goto done; }
        depth--;
        t = st[depth].t; s = st[depth].s; memcpy(mask, st[depth].m, sizeof mask); start = st[depth].i + 1;
    }
done:
    out[0] = memo.n; out[1] = verdict; out[3] = stall_max;
    cset_free(&memo); free(st); orc_key_free(&kk);
    return 0;
}
