/*
 * test_seed_update.c -- the algebra of the streaming batch calls
 * (mchecksum_gpu_update_offsets / state_get / combine), checked on the CPU
 * with the functions the kernels run (crc_gpu_seed.h) and host-built shift
 * packs, for crc32c, crc32, crc64 and the MSB-first crc64-ecma182:
 *  1. the update identity R(s, M) = R(init, M) ^ Z^n(s ^ init), chained over
 *     a random 3-way split of a buffer (R(init, part) from the streaming
 *     API), equals the streaming API over the whole buffer -- and so does
 *     every prefix; state_init + state_get is the CRC of the empty message;
 *  2. the combine formula equals the streaming API over A || B, len_b = 0
 *     and the MSB-first value mapping included.
 */
#include <mchecksum.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "crc_gpu_seed.h"

static uint64_t rng = 0xD1B54A32D192ED03ull;
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

/* the kernels' epilogue: state advanced over a chunk whose R(init, chunk) is x */
static uint64_t seed(const ctx_t *c, uint64_t x, uint64_t s, uint64_t n) {
    return c->w == 32 ? mck_seed32(c->sp, (uint32_t) x, (uint32_t) s, (uint32_t) c->rm.rinit, n)
                      : mck_seed64(c->sp, x, s, c->rm.rinit, n);
}
static uint64_t to_reg(const ctx_t *c, uint64_t v) {
    return c->w == 32 ? mck_crc_to_reg32((uint32_t) v, (uint32_t) c->rm.xorout, c->rm.msb)
                      : mck_crc_to_reg64(v, c->rm.xorout, c->rm.msb);
}
static uint64_t to_crc(const ctx_t *c, uint64_t r) {
    return c->w == 32 ? mck_reg_to_crc32((uint32_t) r, (uint32_t) c->rm.xorout, c->rm.msb)
                      : mck_reg_to_crc64(r, c->rm.xorout, c->rm.msb);
}
static uint64_t combine(const ctx_t *c, uint64_t a, uint64_t b, uint64_t len_b) {
    return c->w == 32 ? mck_combine32(c->sp, (uint32_t) a, (uint32_t) b, len_b, (uint32_t) c->rm.rinit,
                                      (uint32_t) c->rm.xorout, c->rm.msb)
                      : mck_combine64(c->sp, a, b, len_b, c->rm.rinit, c->rm.xorout, c->rm.msb);
}

int main(void) {
    static const char *methods[] = {"crc32c", "crc32", "crc64", "crc64-ecma182"};
    static const size_t fixed[] = {0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 255, 256, 4096, 65536, 65537, 0x10001};
    const size_t nfixed = sizeof(fixed) / sizeof(fixed[0]), cap = 300000;
    int fails = 0, msb_seen = 0;
    unsigned char *buf = malloc(cap);
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
        /* state_init then state_get: the CRC of the empty message */
        if (to_crc(&c, c.rm.rinit) != api_crc(method, buf, 0)) {
            printf("FAIL %s: empty message\n", method);
            fails++;
        }
        for (size_t t = 0; t < nfixed + 60; t++) {
            const size_t n = t < nfixed ? fixed[t] : next() % cap;
            const unsigned char *p = buf + next() % (cap - n + 1);
            /* 1. three chunks, any of them possibly empty */
            size_t c1 = next() % (n + 1), c2 = next() % (n + 1);
            if (c1 > c2) {
                const size_t x = c1;
                c1 = c2;
                c2 = x;
            }
            if (t % 5 == 0) c1 = 0;      /* an empty first chunk */
            if (t % 7 == 0) c2 = c1;     /* an empty middle chunk */
            const size_t cut[4] = {0, c1, c2, n};
            uint64_t s = c.rm.rinit;
            for (int k = 0; k < 3; k++) {
                const size_t len = cut[k + 1] - cut[k];
                const uint64_t before = s;
                s = seed(&c, to_reg(&c, api_crc(method, p + cut[k], len)), s, len);
                if (len == 0 && s != before) {
                    printf("FAIL %s: an empty chunk changed the state\n", method);
                    fails++;
                }
                if (to_crc(&c, s) != api_crc(method, p, cut[k + 1])) {
                    printf("FAIL %s: update n=%zu cuts %zu %zu after chunk %d\n", method, n, c1, c2, k);
                    fails++;
                }
            }
            /* 2. combine: A = p[0, c2), B = p[c2, n), and len_b = 0 */
            if (combine(&c, api_crc(method, p, c2), api_crc(method, p + c2, n - c2), n - c2) != api_crc(method, p, n)) {
                printf("FAIL %s: combine n=%zu len_b=%zu\n", method, n, n - c2);
                fails++;
            }
            if (combine(&c, api_crc(method, p, n), api_crc(method, p, 0), 0) != api_crc(method, p, n)) {
                printf("FAIL %s: combine n=%zu len_b=0\n", method, n);
                fails++;
            }
        }
        free(c.sp);
    }
    free(buf);
    if (!msb_seen) {
        printf("FAIL no MSB-first model among the methods\n");
        fails++;
    }
    if (fails)
        return 1;
    printf("seed update/combine: all checks passed\n");
    return 0;
}
