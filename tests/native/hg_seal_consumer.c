/*
 * hg_seal_consumer.c -- a compiled SENDER on the batch ABI (<mchecksum_gpu.h>),
 * the counterpart of hg_verify_consumer.c: the
 * arguments of NMSG requests sit serialized in device memory, back to back;
 * the program fills the core-header fields of the send buffer, then on a
 * hipStream_t of its own
 *   mchecksum_gpu_pack_messages     copies every payload behind its headers,
 *                                   hashes it and stores the hash network
 *                                   order in the HG header (what HG_PROC_TYPE's
 *                                   memcpy + mchecksum_update and hg_set_struct
 *                                   do, src/mercury_proc.h:124-181,
 *                                   src/mercury.c:699-707),
 *   mchecksum_gpu_seal_core_headers stores the core headers' CRC16
 *                                   (hg_core_header_request_proc, HG_ENCODE,
 *                                   src/mercury_core_header.c:175-230),
 * and the receiver's two verify calls run on the result.  Every payload hash
 * is then compared with hg_proc's streaming sequence on the host (one
 * mchecksum_update per field, mchecksum_get(FINALIZE)), every core-header
 * hash with the per-field CRC16, and every payload byte with the source.
 *
 * Without a HIP device every entry point must refuse with
 * MCHECKSUM_GPU_ENODEV; the program then prints NODEV and exits 0.
 * Exit status: 0 pass, non-zero the failed step.
 */
#include <mchecksum.h>
#include <mchecksum_gpu.h>

#include <hip/hip_runtime_api.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define NMSG 4096
#define HDR 16
#define HGH 4

static uint64_t rng_state = 0x4D43310000000007ull;
static uint64_t
next_u64(void)
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* The payload hash as hg_proc builds it: the u32 length field, then the raw
 * bytes, each through its own mchecksum_update; finalized by hg_proc_flush. */
static int
proc_hash(const uint8_t *p, size_t n, uint32_t *out)
{
    mchecksum_object_t c = MCHECKSUM_OBJECT_NULL;
    const size_t head = n < 4 ? n : 4;
    if (mchecksum_init("crc32c", &c) != 0)
        return -1;
    if (head && mchecksum_update(c, p, head) != 0)
        return -1;
    if (n > head && mchecksum_update(c, p + head, n - head) != 0)
        return -1;
    if (mchecksum_get(c, out, sizeof(*out), MCHECKSUM_FINALIZE) != 0)
        return -1;
    return mchecksum_destroy(c);
}

static uint16_t
core_header_crc16(uint8_t hg, uint8_t protocol, uint64_t id, uint8_t flags, uint8_t cookie)
{
    mchecksum_object_t c = MCHECKSUM_OBJECT_NULL;
    uint16_t h = 0;
    if (mchecksum_init("crc16", &c) != 0)
        return 0;
    mchecksum_update(c, &hg, 1);
    mchecksum_update(c, &protocol, 1);
    mchecksum_update(c, &id, 8); /* host order */
    mchecksum_update(c, &flags, 1);
    mchecksum_update(c, &cookie, 1);
    mchecksum_get(c, &h, sizeof(h), MCHECKSUM_FINALIZE);
    mchecksum_destroy(c);
    return h;
}

static void
put_be(uint8_t *p, uint64_t v, int n)
{
    for (int k = 0; k < n; k++)
        p[k] = (uint8_t)(v >> (8 * (n - 1 - k)));
}
static uint64_t
get_be(const uint8_t *p, int n)
{
    uint64_t v = 0;
    for (int k = 0; k < n; k++)
        v = v << 8 | p[k];
    return v;
}

#define HIPCHK(x)                                                               \
    do {                                                                        \
        hipError_t e_ = (x);                                                    \
        if (e_ != hipSuccess) {                                                 \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));             \
            return 20;                                                          \
        }                                                                       \
    } while (0)

int
main(void)
{
    if (!mchecksum_gpu_available()) {
        uint8_t st = 0;
        uint64_t off[2] = {0, 0};
        int rc1 = mchecksum_gpu_pack_messages("crc32c", off, off, off, off, 1, HDR + HGH, HDR, &st, NULL);
        int rc2 = mchecksum_gpu_seal_messages("crc32c", off, off, 1, HDR + HGH, HDR, &st, NULL);
        int rc3 = mchecksum_gpu_seal_core_headers("crc16", MCHECKSUM_GPU_CORE_HEADER_REQUEST, off, off, 1, &st, NULL);
        if (rc1 != MCHECKSUM_GPU_ENODEV || rc2 != MCHECKSUM_GPU_ENODEV || rc3 != MCHECKSUM_GPU_ENODEV) {
            fprintf(stderr, "no device, but rc %d / %d / %d\n", rc1, rc2, rc3);
            return 2;
        }
        printf("NODEV: pack_messages, seal_messages and seal_core_headers refused with MCHECKSUM_GPU_ENODEV\n");
        return 0;
    }

    /* the device argument buffer (payloads 0 B .. 16 KiB, byte-packed) and the send buffer's message table */
    uint64_t *so = malloc((NMSG + 1) * sizeof(uint64_t)), *mo = malloc((NMSG + 1) * sizeof(uint64_t));
    so[0] = 3;
    mo[0] = 0;
    for (size_t i = 0; i < NMSG; i++) {
        size_t pay = (size_t)(next_u64() % 16385);
        if (i % 97 == 5)
            pay = 0;
        so[i + 1] = so[i] + pay;
        mo[i + 1] = mo[i] + HDR + HGH + pay;
    }
    const size_t src_bytes = so[NMSG], total = mo[NMSG];
    uint8_t *src = malloc(src_bytes + 64), *buf = malloc(total);
    for (size_t k = 0; k < src_bytes + 64; k++)
        src[k] = (uint8_t) next_u64();
    /* the sender fills the core-header fields; both hash fields and the payload are the library's to write */
    memset(buf, 0xEE, total);
    for (size_t i = 0; i < NMSG; i++) {
        uint8_t *m = buf + mo[i];
        m[0] = 'H' << 1 | 1;
        m[1] = 4;
        put_be(m + 2, next_u64(), 8);
        m[10] = (uint8_t) i;
        m[11] = (uint8_t)(i >> 8);
        m[12] = m[13] = 0xFF;
        m[14] = m[15] = 0;
    }

    void *d_src = NULL, *d_so = NULL, *d_buf = NULL, *d_mo = NULL, *d_st = NULL, *d_cnt = NULL;
    hipStream_t s;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&d_src, src_bytes + 64));
    HIPCHK(hipMalloc(&d_buf, total));
    HIPCHK(hipMalloc(&d_so, (NMSG + 1) * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&d_mo, (NMSG + 1) * sizeof(uint64_t)));
    HIPCHK(hipMalloc(&d_st, 4 * NMSG));
    HIPCHK(hipMalloc(&d_cnt, 2 * sizeof(uint32_t)));
    HIPCHK(hipMemcpyAsync(d_src, src, src_bytes + 64, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_buf, buf, total, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_so, so, (NMSG + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_mo, mo, (NMSG + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_cnt, 0, 2 * sizeof(uint32_t), s));
    HIPCHK(hipMemsetAsync(d_st, 1, 4 * NMSG, s));
    if (mchecksum_gpu_prepare("crc32c") != MCHECKSUM_GPU_OK || mchecksum_gpu_prepare("crc16") != MCHECKSUM_GPU_OK) {
        fprintf(stderr, "prepare: %s\n", mchecksum_gpu_last_error());
        return 5;
    }
    uint8_t *d_st_pack = d_st, *d_st_seal = (uint8_t *) d_st + NMSG, *d_st_hdr = (uint8_t *) d_st + 2 * NMSG,
            *d_st_pay = (uint8_t *) d_st + 3 * NMSG;
    uint32_t *d_nhdr = d_cnt, *d_npay = (uint32_t *) d_cnt + 1;
    int rc = mchecksum_gpu_pack_messages("crc32c", d_src, d_so, d_buf, d_mo, NMSG, HDR + HGH, HDR, d_st_pack, s);
    if (rc != MCHECKSUM_GPU_OK) {
        fprintf(stderr, "pack_messages rc %d: %s\n", rc, mchecksum_gpu_last_error());
        return 6;
    }
    rc = mchecksum_gpu_seal_core_headers("crc16", MCHECKSUM_GPU_CORE_HEADER_REQUEST, d_buf, d_mo, NMSG, d_st_seal, s);
    if (rc != MCHECKSUM_GPU_OK) {
        fprintf(stderr, "seal_core_headers rc %d: %s\n", rc, mchecksum_gpu_last_error());
        return 7;
    }
    /* the receiver's side, on the same stream */
    rc = mchecksum_gpu_verify_core_headers("crc16", MCHECKSUM_GPU_CORE_HEADER_REQUEST, d_buf, d_mo, NMSG, d_st_hdr,
                                           d_nhdr, s);
    if (rc == MCHECKSUM_GPU_OK)
        rc = mchecksum_gpu_verify_messages("crc32c", d_buf, d_mo, NMSG, HDR + HGH, HDR, d_st_pay, d_npay, s);
    if (rc != MCHECKSUM_GPU_OK) {
        fprintf(stderr, "verify rc %d: %s\n", rc, mchecksum_gpu_last_error());
        return 8;
    }
    uint8_t *got = malloc(total), *st = malloc(4 * NMSG);
    uint32_t cnt[2];
    HIPCHK(hipMemcpyAsync(got, d_buf, total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(st, d_st, 4 * NMSG, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));

    size_t flagged = 0, bad_pay_hash = 0, bad_hdr_hash = 0, bad_bytes = 0, bad_fields = 0;
    for (size_t i = 0; i < 4 * NMSG; i++)
        flagged += st[i] != 0;
    for (size_t i = 0; i < NMSG; i++) {
        const uint8_t *m = got + mo[i], *was = buf + mo[i];
        const size_t pay = so[i + 1] - so[i];
        uint32_t h = 0, wire = (uint32_t) get_be(m + HDR, 4);
        if (proc_hash(src + so[i], pay, &h) != 0)
            return 9;
        bad_pay_hash += memcmp(&h, &wire, sizeof(h)) != 0;
        bad_hdr_hash += core_header_crc16(m[0], m[1], get_be(m + 2, 8), m[10], m[11]) != (uint16_t) get_be(m + 12, 2);
        bad_bytes += memcmp(m + HDR + HGH, src + so[i], pay) != 0;
        bad_fields += memcmp(m, was, 12) != 0 || m[14] != was[14] || m[15] != was[15];
        if ((memcmp(&h, &wire, sizeof(h)) != 0) && bad_pay_hash <= 4)
            fprintf(stderr, "message %zu (%zu payload bytes): stored hash %08x, hg_proc's %08x\n", i, pay, wire, h);
    }
    printf("gpu sender: %d messages (%zu bytes) packed on a hipStream_t: payload hashes %zu differ, core-header hashes "
           "%zu differ, payloads %zu differ, header fields %zu changed; statuses flagged %zu; receiver flagged %u / %u\n",
           NMSG, total, bad_pay_hash, bad_hdr_hash, bad_bytes, bad_fields, flagged, cnt[0], cnt[1]);
    if (bad_pay_hash || bad_hdr_hash || bad_bytes || bad_fields || flagged || cnt[0] || cnt[1])
        return 10;
    HIPCHK(hipFree(d_src));
    HIPCHK(hipFree(d_buf));
    HIPCHK(hipFree(d_so));
    HIPCHK(hipFree(d_mo));
    HIPCHK(hipFree(d_st));
    HIPCHK(hipFree(d_cnt));
    HIPCHK(hipStreamDestroy(s));
    printf("PASS\n");
    return 0;
}
