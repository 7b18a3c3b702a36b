/*
 * test_seg_update.c -- the algebra of the streaming segment calls
 * (mchecksum_gpu_update_segments / _update_gather_segments /
 * _update_scatter_segments), checked on the CPU with the functions the
 * kernels run (crc_gpu_seed.h) against the oracle's streaming register
 * (oracle/crc_oracle.c), for crc32c, crc32, crc64-xz, crc64-ecma182 and
 * crc64-jones.
 *
 * A random byte string is cut into 1-5 stages and each stage into 0-4
 * segments (lengths 0, 1, W/8 - 1 and W/8 among them).  A stage is what one
 * update call sees: the state's word is preset with the seed term of the
 * stage's byte total N (mck_seg_seed, what seg_pre_kernel stores), then every
 * segment XORs its contribution into it as the chunk pass does (seg_emit): its
 * zero-init register shifted over the bytes after it, and for the head
 * segment the object term Z^N(init) ^ init.  After every stage the word,
 * finalised, must equal the oracle's streaming CRC of all bytes so far; a
 * stage without bytes must leave it bit-identical.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crc_gpu_seed.h"
#include "crc_oracle.h"

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next(void) {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
}

typedef struct {
    int w;
    crc_rmodel_t rm;
    void *sp;
} ctx_t;

static uint64_t zshift(const ctx_t *c, uint64_t x, uint64_t n) {
    return c->w == 32 ? mck_zshift32(c->sp, (uint32_t) x, n) : mck_zshift64(c->sp, x, n);
}
static uint64_t seg_seed(const ctx_t *c, uint64_t s, uint64_t n) {
    return c->w == 32 ? mck_seg_seed32(c->sp, (uint32_t) s, (uint32_t) c->rm.rinit, n)
                      : mck_seg_seed64(c->sp, s, c->rm.rinit, n);
}
static uint64_t to_reg(const ctx_t *c, uint64_t v) {
    return c->w == 32 ? mck_crc_to_reg32((uint32_t) v, (uint32_t) c->rm.xorout, c->rm.msb)
                      : mck_crc_to_reg64(v, c->rm.xorout, c->rm.msb);
}
static uint64_t to_crc(const ctx_t *c, uint64_t r) {
    return c->w == 32 ? mck_reg_to_crc32((uint32_t) r, (uint32_t) c->rm.xorout, c->rm.msb)
                      : mck_reg_to_crc64(r, c->rm.xorout, c->rm.msb);
}
/* the value verify_segments compares: from the XOR of the contributions alone */
static uint64_t seg_value(const ctx_t *c, uint64_t x) {
    return c->w == 32 ? mck_seg_value32((uint32_t) x, (uint32_t) c->rm.rinit, (uint32_t) c->rm.xorout, c->rm.msb)
                      : mck_seg_value64(x, c->rm.rinit, c->rm.xorout, c->rm.msb);
}

/* a length: one of the edge lengths of a W-bit register, or anything up to cap */
static size_t pick_len(int w, size_t cap) {
    const size_t edge[] = {0, 1, (size_t) w / 8 - 1, (size_t) w / 8, (size_t) w / 8 + 1};
    const uint64_t r = next();
    size_t n = r % 3 == 0 ? edge[(r >> 8) % 5] : (size_t) ((r >> 8) % (cap + 1));
    return n > cap ? cap : n;
}

int main(void) {
    static const char *methods[] = {"crc32c", "crc32", "crc64-xz", "crc64-ecma182", "crc64-jones"};
    const size_t cap = 6000;
    int fails = 0, msb_seen = 0;
    long stages_run = 0, empty_stages = 0, segs_run = 0;
    unsigned char *buf = malloc(cap);
    for (size_t i = 0; i < cap; i++) buf[i] = (unsigned char) next();
    for (int mi = 0; mi < 5; mi++) {
        const char *method = methods[mi];
        const mck_model_t *m = &mck_models[mck_model_index(method)];
        const oracle_model_t *om = oracle_model_by_name(method);
        ctx_t c = {m->width, mck_gpu_rmodel(m), NULL};
        if (!om || om->width != c.w) {
            printf("FAIL the oracle has no %s\n", method);
            return 1;
        }
        c.sp = calloc(1, c.w == 32 ? sizeof(crc32_shift_pack_t) : sizeof(crc64_shift_pack_t));
        if ((c.w == 32 ? crc32_shift_pack_build(&c.rm, c.sp) : crc64_shift_pack_build(&c.rm, c.sp)) != 0) {
            printf("FAIL shift pack build %s\n", method);
            return 1;
        }
        msb_seen |= c.rm.msb;
        for (int t = 0; t < 300; t++) {
            const int nstages = 1 + (int) (next() % 5);
            size_t used = 0;
            uint64_t s = c.rm.rinit;                 /* state_init */
            uint64_t oreg = oracle_reg_init(om);     /* the oracle's stream */
            for (int st = 0; st < nstages; st++) {
                const int nsegs = t % 11 == 0 && st == 1 ? 0 : (int) (next() % 5);
                size_t len[4], at[4], N = 0;
                for (int i = 0; i < nsegs; i++) {
                    /* an all-empty stage now and then; otherwise mixed lengths */
                    len[i] = t % 7 == 0 && st == 0 ? 0 : pick_len(c.w, (cap - used - N) / 2);
                    at[i] = used + N;
                    N += len[i];
                }
                const uint64_t before = s;
                uint64_t word = N ? seg_seed(&c, s, N) : s; /* (N = 0: the kernel does not write) */
                if (seg_seed(&c, s, 0) != s) {
                    printf("FAIL %s: the seed term of no bytes is not the state\n", method);
                    fails++;
                }
                uint64_t x = 0; /* the contributions alone, as verify_segments accumulates them */
                int head_seen = 0;
                size_t after = N;
                for (int i = 0; i < nsegs; i++) {
                    const size_t n = len[i];
                    after -= n;
                    if (!n) continue; /* an empty segment has no chunk */
                    /* L(seg) = R(init, seg) ^ Z^n(init), R(init, seg) from the oracle */
                    const uint64_t r = to_reg(&c, oracle_crc_bitwise(om, buf + at[i], n));
                    uint64_t contrib = zshift(&c, r ^ zshift(&c, c.rm.rinit, n), after);
                    if (!head_seen) { /* the head chunk carries the object term, and init once more */
                        contrib ^= zshift(&c, c.rm.rinit, n + after) ^ c.rm.rinit;
                        head_seen = 1;
                    }
                    x ^= contrib;
                    oreg = oracle_reg_update(om, oreg, buf + at[i], n);
                    segs_run++;
                }
                s = word ^ x;
                used += N;
                stages_run++;
                if (N == 0) {
                    empty_stages++;
                    if (s != before) {
                        printf("FAIL %s: a stage without bytes changed the state\n", method);
                        fails++;
                    }
                }
                if (to_crc(&c, s) != oracle_reg_final(om, oreg)) {
                    printf("FAIL %s: trial %d stage %d of %d, N=%zu\n", method, t, st, nstages, N);
                    fails++;
                }
                /* one-shot: the contributions alone give this stage's own CRC */
                if (seg_value(&c, x) != oracle_crc_bitwise(om, buf + used - N, N)) {
                    printf("FAIL %s: trial %d stage %d one-shot value, N=%zu\n", method, t, st, N);
                    fails++;
                }
            }
        }
        free(c.sp);
    }
    free(buf);
    if (!msb_seen) {
        printf("FAIL no MSB-first model among the methods\n");
        fails++;
    }
    if (!empty_stages || segs_run < 1000) {
        printf("FAIL vacuous run: %ld empty stages, %ld segments\n", empty_stages, segs_run);
        fails++;
    }
    if (fails) return 1;
    printf("%ld stages (%ld without bytes), %ld segments\n", stages_run, empty_stages, segs_run);
    printf("segment update algebra: all checks passed\n");
    return 0;
}
