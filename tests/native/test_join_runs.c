/*
 * test_join_runs.c -- the join of mchecksum_gpu_combine_runs, checked on the
 * CPU with the functions the kernel runs (crc_gpu_seed.h: mck_join_in /
 * mck_join / mck_join_out) and host-built shift packs, for crc32c, crc32,
 * crc64 and the MSB-first crc64-ecma182.  A random buffer is cut into random
 * chunks (zero-length ones included, their CRC words garbage); the chunk CRCs
 * come from the streaming API; the run's CRC must equal mchecksum_update over
 * the bytes when the elements are joined
 *  1. left to right,
 *  2. as a balanced tree,
 *  3. in a random bracketing,
 *  4. in the kernel's bracketing: W lanes fold contiguous slices of
 *     ceil(K / W) chunks, then a shuffle-down tree (W = 64; W = 256 as four
 *     waves joined left to right),
 * each keeping the chunks in order; the joined length is the byte total; and
 * one more zero-length chunk with a garbage CRC word, anywhere, changes
 * nothing.  The identity joined with the identity is the empty message.
 */
#include <mchecksum.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crc_gpu_seed.h"

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next(void) {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
}

static uint64_t api_crc(const char *method, const unsigned char *p, size_t n) {
    mchecksum_object_t c = MCHECKSUM_OBJECT_NULL;
    uint64_t v = 0;
    mchecksum_init(method, &c);
    mchecksum_update(c, p, n);
    mchecksum_get(c, &v, mchecksum_get_size(c), MCHECKSUM_FINALIZE);
    mchecksum_destroy(c);
    return v;
}

typedef struct {
    int w;
    crc_rmodel_t rm;
    void *sp;
} ctx_t;

/* one element type for both widths: the 32-bit functions on the low half */
typedef mck_join64_t elem_t;

static elem_t el_in(const ctx_t *c, uint64_t v, uint64_t n) {
    if (c->w == 32) {
        const mck_join32_t e = mck_join_in32((uint32_t) v, n, (uint32_t) c->rm.rinit, (uint32_t) c->rm.xorout, c->rm.msb);
        const elem_t r = {e.r, e.n};
        return r;
    }
    return mck_join_in64(v, n, c->rm.rinit, c->rm.xorout, c->rm.msb);
}
static elem_t el_join(const ctx_t *c, elem_t a, elem_t b) {
    if (c->w == 32) {
        const mck_join32_t a32 = {(uint32_t) a.r, a.n}, b32 = {(uint32_t) b.r, b.n};
        const mck_join32_t e = mck_join32(c->sp, a32, b32, (uint32_t) c->rm.rinit);
        const elem_t r = {e.r, e.n};
        return r;
    }
    return mck_join64(c->sp, a, b, c->rm.rinit);
}
static uint64_t el_out(const ctx_t *c, elem_t e) {
    if (c->w == 32) {
        const mck_join32_t e32 = {(uint32_t) e.r, e.n};
        return mck_join_out32(e32, (uint32_t) c->rm.xorout, c->rm.msb);
    }
    return mck_join_out64(e, c->rm.xorout, c->rm.msb);
}
static elem_t el_identity(const ctx_t *c) { return el_in(c, 0xA5A5A5A5A5A5A5A5ull, 0); }

static elem_t fold_left(const ctx_t *c, const elem_t *e, size_t k) {
    elem_t acc = el_identity(c);
    for (size_t i = 0; i < k; i++) acc = el_join(c, acc, e[i]);
    return acc;
}
static elem_t fold_balanced(const ctx_t *c, const elem_t *e, size_t k) {
    if (k == 0) return el_identity(c);
    if (k == 1) return e[0];
    return el_join(c, fold_balanced(c, e, k / 2), fold_balanced(c, e + k / 2, k - k / 2));
}
static elem_t fold_random(const ctx_t *c, const elem_t *e, size_t k) {
    if (k == 0) return el_identity(c);
    if (k == 1) return e[0];
    const size_t cut = 1 + next() % (k - 1);
    return el_join(c, fold_random(c, e, cut), fold_random(c, e + cut, k - cut));
}
/* the kernel's wave: 64 lanes' elements, step d joins lane l (a multiple of 2d) with lane l + d */
static elem_t wave_tree(const ctx_t *c, elem_t *lane) {
    for (int d = 1; d < 64; d <<= 1)
        for (int l = 0; l < 64; l += 2 * d) lane[l] = el_join(c, lane[l], lane[l + d]);
    return lane[0];
}
/* the kernel's bracketing with `width` lanes (64: one wave; 256: four waves, joined through LDS) */
static elem_t fold_kernel(const ctx_t *c, const elem_t *e, size_t k, size_t width) {
    elem_t lanes[256], acc;
    const size_t m = (k + width - 1) / width;
    for (size_t l = 0; l < width; l++) {
        const size_t s0 = l * m < k ? l * m : k, s1 = l * m + m < k ? l * m + m : k;
        lanes[l] = s0 < s1 ? e[s0] : el_identity(c);
        for (size_t i = s0 + 1; i < s1; i++) lanes[l] = el_join(c, lanes[l], e[i]);
    }
    acc = wave_tree(c, lanes);
    for (size_t v = 1; v < width / 64; v++) acc = el_join(c, acc, wave_tree(c, lanes + 64 * v));
    return acc;
}

#define MAXK 700

int main(void) {
    static const char *methods[] = {"crc32c", "crc32", "crc64", "crc64-ecma182"};
    static const size_t pool[] = {0, 0, 1, 2, 3, 7, 8, 15, 16, 17, 255, 256, 257, 4096, 4097};
    static const size_t counts[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, MAXK - 1};
    const size_t npool = sizeof(pool) / sizeof(pool[0]), ncounts = sizeof(counts) / sizeof(counts[0]);
    const size_t cap = MAXK * 4097;
    int fails = 0, msb_seen = 0;
    unsigned char *buf = malloc(cap);
    elem_t *e = malloc((MAXK + 1) * sizeof(*e));
    for (size_t i = 0; i < cap; i++) buf[i] = (unsigned char) next();
    for (int mi = 0; mi < 4; mi++) {
        const char *method = methods[mi];
        const mck_model_t *m = &mck_models[mck_model_index(method)];
        ctx_t c = {m->width, mck_gpu_rmodel(m), NULL};
        c.sp = calloc(1, c.w == 32 ? sizeof(crc32_shift_pack_t) : sizeof(crc64_shift_pack_t));
        if ((c.w == 32 ? crc32_shift_pack_build(&c.rm, c.sp) : crc64_shift_pack_build(&c.rm, c.sp)) != 0) {
            printf("FAIL shift pack build %s\n", method);
            return 1;
        }
        msb_seen |= c.rm.msb;
        if (el_out(&c, el_join(&c, el_identity(&c), el_identity(&c))) != api_crc(method, buf, 0)) {
            printf("FAIL %s: identity o identity is not the empty message\n", method);
            fails++;
        }
        for (size_t t = 0; t < ncounts + 24; t++) {
            const size_t k = t < ncounts ? counts[t] : next() % MAXK;
            size_t total = 0, nzero = 0;
            for (size_t i = 0; i < k; i++) {
                /* short chunks mostly; every fifth from the pool; t % 4 == 3: half of them empty */
                size_t n = next() % 5 == 0 ? pool[next() % npool] : next() % 200;
                if (t % 4 == 3 && next() % 2) n = 0;
                /* a zero-length chunk carries a garbage CRC word */
                e[i] = el_in(&c, n ? api_crc(method, buf + total, n) : next(), n);
                total += n;
                nzero += n == 0;
            }
            const uint64_t want = api_crc(method, buf, total);
            const struct {
                const char *name;
                elem_t v;
            } folds[] = {{"left fold", fold_left(&c, e, k)},         {"balanced tree", fold_balanced(&c, e, k)},
                         {"random bracketing", fold_random(&c, e, k)}, {"kernel, one wave", fold_kernel(&c, e, k, 64)},
                         {"kernel, workgroup", fold_kernel(&c, e, k, 256)}};
            for (size_t f = 0; f < sizeof(folds) / sizeof(folds[0]); f++)
                if (el_out(&c, folds[f].v) != want || folds[f].v.n != total) {
                    printf("FAIL %s: %s of %zu chunks (%zu empty), %zu bytes\n", method, folds[f].name, k, nzero, total);
                    fails++;
                }
            /* one more zero-length chunk with a garbage word, at a random place */
            const size_t at = next() % (k + 1);
            memmove(e + at + 1, e + at, (k - at) * sizeof(*e));
            e[at] = el_in(&c, 0xA5A5A5A5A5A5A5A5ull ^ next(), 0);
            if (el_out(&c, fold_left(&c, e, k + 1)) != want || el_out(&c, fold_random(&c, e, k + 1)) != want ||
                el_out(&c, fold_kernel(&c, e, k + 1, 64)) != want) {
                printf("FAIL %s: a zero-length chunk at %zu of %zu changed the value\n", method, at, k);
                fails++;
            }
        }
        free(c.sp);
    }
    free(e);
    free(buf);
    if (!msb_seen) {
        printf("FAIL no MSB-first model among the methods\n");
        fails++;
    }
    if (fails)
        return 1;
    printf("join runs: all checks passed\n");
    return 0;
}
