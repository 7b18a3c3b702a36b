/*
 * crc_gpu_seed.h -- the algebra of the streaming batch calls
 * (mchecksum_gpu_state_init / update_offsets / state_get / combine /
 * combine_runs), shared verbatim by the HIP kernels and the CPU tests
 * tests/native/test_seed_update.c and test_join_runs.c so the CPU checks the
 * exact code the GPU runs.
 *
 * R(s, M) is the register after hashing the n bytes of M starting from
 * register s (crc_gpu_layout.h: reflected form; an MSB-first model in its
 * byte-reversed R domain).  The register is affine in s with linear part Z^n:
 *
 *     R(s, M) = R(init, M) ^ Z^n(s ^ init)
 *
 * R(init, M) is what the offsets kernels hold just before they emit
 * x ^ xorout, so a seeded update is the unseeded payload loop plus one Z^n on
 * the lane that owns the payload.  Two finalized CRCs join the same way:
 * CRC(A || B) comes from R(init, B) ^ Z^|B|(R(init, A) ^ init).
 *
 * Z^n comes from the base-16 digit tables of the shift pack
 * (crc32/64_shift_pack_build): CRC_SHIFT_DIGITS digits, n < 2^48.  The digit
 * loop is bounded by the pack, so a larger n reads nothing out of range (its
 * high digits are ignored and the value is then unspecified).
 */
#ifndef CRC_GPU_SEED_H
#define CRC_GPU_SEED_H

#include <stdint.h>

#include "crc_gpu_layout.h"
#include "crc_gpu_mask.h" /* MCK_HD */
#include "mchecksum_models.h"

MCK_HD uint32_t
mck_zshift32(const crc32_shift_pack_t *sp, uint32_t x, uint64_t n)
{
    for (int k = 0; k < CRC_SHIFT_DIGITS && n; k++, n >>= 4) {
        const uint32_t d = (uint32_t) (n & 15u);
        if (d) {
            const uint32_t *t = &sp->op[k][d - 1][0][0];
            uint32_t r = 0;
            for (int h = 0; h < 8; h++)
                r ^= t[h * 16 + ((x >> (4 * h)) & 15u)];
            x = r;
        }
    }
    return x;
}

MCK_HD uint64_t
mck_zshift64(const crc64_shift_pack_t *sp, uint64_t x, uint64_t n)
{
    for (int k = 0; k < CRC_SHIFT_DIGITS && n; k++, n >>= 4) {
        const uint32_t d = (uint32_t) (n & 15u);
        if (d) {
            const uint64_t *t = &sp->op[k][d - 1][0][0];
            uint64_t r = 0;
            for (int h = 0; h < 16; h++)
                r ^= t[h * 16 + ((x >> (4 * h)) & 15u)];
            x = r;
        }
    }
    return x;
}

/* The seeded update: x = R(init, M), |M| = n, s = the running register
 * before M; returns R(s, M).  n = 0 (x = init) returns s. */
MCK_HD uint32_t
mck_seed32(const crc32_shift_pack_t *sp, uint32_t x, uint32_t s, uint32_t init, uint64_t n)
{
    return x ^ mck_zshift32(sp, s ^ init, n);
}

MCK_HD uint64_t
mck_seed64(const crc64_shift_pack_t *sp, uint64_t x, uint64_t s, uint64_t init, uint64_t n)
{
    return x ^ mck_zshift64(sp, s ^ init, n);
}

/* The segment passes (mchecksum_gpu_ext.hip) XOR into an object's word what
 * its chunks contribute: R(init, M) ^ init between them for an object of
 * N > 0 bytes (the head chunk adds the init once more, seg_emit), nothing for
 * one without bytes.  A segments update presets the word with the seed term
 * so that it ends as R(s, M) -- s itself for N = 0, which the caller need not
 * write: */
MCK_HD uint32_t
mck_seg_seed32(const crc32_shift_pack_t *sp, uint32_t s, uint32_t init, uint64_t n)
{
    return init ^ mck_zshift32(sp, s ^ init, n);
}

MCK_HD uint64_t
mck_seg_seed64(const crc64_shift_pack_t *sp, uint64_t s, uint64_t init, uint64_t n)
{
    return init ^ mck_zshift64(sp, s ^ init, n);
}

/* Register <-> finalized value (what mchecksum_get() returns).  The kernels'
 * value of an MSB-first model is the CRC byte-swapped (crc_gpu_layout.h);
 * xorout is the model's in the kernels' domain (crc_rmodel_t). */
MCK_HD uint32_t
mck_reg_to_crc32(uint32_t r, uint32_t xorout, int msb)
{
    r ^= xorout;
    return msb ? __builtin_bswap32(r) : r;
}

MCK_HD uint64_t
mck_reg_to_crc64(uint64_t r, uint64_t xorout, int msb)
{
    r ^= xorout;
    return msb ? __builtin_bswap64(r) : r;
}

/* The finalized CRC of an object from x, the XOR of its chunks' contributions
 * into a zeroed word (mck_seg_seed above): 0 for the empty message. */
MCK_HD uint32_t
mck_seg_value32(uint32_t x, uint32_t init, uint32_t xorout, int msb)
{
    return mck_reg_to_crc32(x ^ init, xorout, msb);
}

MCK_HD uint64_t
mck_seg_value64(uint64_t x, uint64_t init, uint64_t xorout, int msb)
{
    return mck_reg_to_crc64(x ^ init, xorout, msb);
}

MCK_HD uint32_t
mck_crc_to_reg32(uint32_t v, uint32_t xorout, int msb)
{
    return (msb ? __builtin_bswap32(v) : v) ^ xorout;
}

MCK_HD uint64_t
mck_crc_to_reg64(uint64_t v, uint64_t xorout, int msb)
{
    return (msb ? __builtin_bswap64(v) : v) ^ xorout;
}

/* CRC(A || B) from a = CRC(A), b = CRC(B) and len_b = |B|. */
MCK_HD uint32_t
mck_combine32(const crc32_shift_pack_t *sp, uint32_t a, uint32_t b, uint64_t len_b, uint32_t init, uint32_t xorout,
              int msb)
{
    const uint32_t ra = mck_crc_to_reg32(a, xorout, msb), rb = mck_crc_to_reg32(b, xorout, msb);
    return mck_reg_to_crc32(mck_seed32(sp, rb, ra, init, len_b), xorout, msb);
}

MCK_HD uint64_t
mck_combine64(const crc64_shift_pack_t *sp, uint64_t a, uint64_t b, uint64_t len_b, uint64_t init, uint64_t xorout,
              int msb)
{
    const uint64_t ra = mck_crc_to_reg64(a, xorout, msb), rb = mck_crc_to_reg64(b, xorout, msb);
    return mck_reg_to_crc64(mck_seed64(sp, rb, ra, init, len_b), xorout, msb);
}

/* The join of mchecksum_gpu_combine_runs: the monoid of (r, n) = (R(init, M),
 * |M|) under concatenation.
 *
 *     identity   (init, 0)                          the empty message
 *     a o b    = (mck_seed(b.r, a.r, init, b.n), a.n + b.n)        A || B
 *
 * Associative (concatenation is), not commutative: a reduction may bracket
 * the chunks of a run any way it likes as long as it keeps them in order.
 * join_in maps a finalized CRC and its byte count to an element -- a
 * zero-length chunk to the identity, whatever its CRC word holds --, join_out
 * an element back to the finalized CRC. */
typedef struct {
    uint32_t r;
    uint64_t n;
} mck_join32_t;

typedef struct {
    uint64_t r;
    uint64_t n;
} mck_join64_t;

MCK_HD mck_join32_t
mck_join_in32(uint32_t v, uint64_t n, uint32_t init, uint32_t xorout, int msb)
{
    mck_join32_t e;
    e.r = n ? mck_crc_to_reg32(v, xorout, msb) : init;
    e.n = n;
    return e;
}

MCK_HD mck_join64_t
mck_join_in64(uint64_t v, uint64_t n, uint64_t init, uint64_t xorout, int msb)
{
    mck_join64_t e;
    e.r = n ? mck_crc_to_reg64(v, xorout, msb) : init;
    e.n = n;
    return e;
}

MCK_HD mck_join32_t
mck_join32(const crc32_shift_pack_t *sp, mck_join32_t a, mck_join32_t b, uint32_t init)
{
    mck_join32_t e;
    e.r = mck_seed32(sp, b.r, a.r, init, b.n);
    e.n = a.n + b.n;
    return e;
}

MCK_HD mck_join64_t
mck_join64(const crc64_shift_pack_t *sp, mck_join64_t a, mck_join64_t b, uint64_t init)
{
    mck_join64_t e;
    e.r = mck_seed64(sp, b.r, a.r, init, b.n);
    e.n = a.n + b.n;
    return e;
}

MCK_HD uint32_t
mck_join_out32(mck_join32_t e, uint32_t xorout, int msb)
{
    return mck_reg_to_crc32(e.r, xorout, msb);
}

MCK_HD uint64_t
mck_join_out64(mck_join64_t e, uint64_t xorout, int msb)
{
    return mck_reg_to_crc64(e.r, xorout, msb);
}

/* Host only: a catalogue model in the kernels' form.  A reflected model as
 * is; an MSB-first model as the reflected model of the same polynomial over
 * bit-reversed bytes, conjugated by R (crc_gpu_layout.h): rinit / xorout
 * reflected, then R-mapped. */
static inline crc_rmodel_t
mck_gpu_rmodel(const mck_model_t *m)
{
    crc_rmodel_t rm;
    rm.width = m->width;
    rm.rpoly = mck_reflect(m->poly, m->width);
    rm.msb = !m->reflected;
    rm.rinit = rm.msb ? crc_rev_bytes(m->width, mck_reflect(m->init, m->width)) : mck_reflect(m->init, m->width);
    rm.xorout = rm.msb ? crc_rev_bytes(m->width, mck_reflect(m->xorout, m->width)) : m->xorout;
    return rm;
}

#endif
