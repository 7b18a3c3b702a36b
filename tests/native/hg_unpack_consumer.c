/*
 * hg_unpack_consumer.c -- a compiled RECEIVER on the batch ABI
 * (<mchecksum_gpu.h>), the counterpart of hg_seal_consumer.c (INTEGRATION.md
 * section 3): NMSG requests are packed into a device receive buffer with
 * mchecksum_gpu_pack_messages, then on a hipStream_t of its own
 *   mchecksum_gpu_unpack_messages   copies every payload out of the receive
 *                                   buffer to where it is consumed and checks
 *                                   its hash in the same pass (what
 *                                   HG_PROC_TYPE on HG_DECODE and hg_get_struct
 *                                   do, src/mercury_proc.h:124-181,
 *                                   src/mercury.c:565-573).
 * The unpacked bytes must equal the source's and every status must read 0.
 * Then one payload bit of one message is flipped in the receive buffer and the
 * call repeated: exactly that message must read 1, one mismatch be counted,
 * and every destination byte equal the bytes as received.
 *
 * Without a HIP device the entry point must refuse with MCHECKSUM_GPU_ENODEV;
 * the program then prints NODEV and exits 0.
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
#define FLIP 1234 /* the message whose payload gets a flipped bit */

static uint64_t rng_state = 0x4D43310000000008ull;
static uint64_t
next_u64(void)
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
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
        int rc = mchecksum_gpu_unpack_messages("crc32c", off, off, 1, HDR + HGH, HDR, off, off, &st, NULL, NULL);
        if (rc != MCHECKSUM_GPU_ENODEV) {
            fprintf(stderr, "no device, but rc %d\n", rc);
            return 2;
        }
        printf("NODEV: unpack_messages refused with MCHECKSUM_GPU_ENODEV\n");
        return 0;
    }

    /* payloads of 0 B .. 16 KiB, byte-packed: so = the source's and the destination's table (the destination
     * starts 5 bytes into its buffer), mo = the receive buffer's message table */
    uint64_t *so = malloc((NMSG + 1) * sizeof(uint64_t)), *mo = malloc((NMSG + 1) * sizeof(uint64_t)),
             *dof = malloc((NMSG + 1) * sizeof(uint64_t));
    so[0] = 3;
    mo[0] = 0;
    dof[0] = 5;
    for (size_t i = 0; i < NMSG; i++) {
        size_t pay = (size_t)(next_u64() % 16385);
        if (i % 97 == 5)
            pay = 0;
        if (i == FLIP && pay < 100)
            pay = 100;
        so[i + 1] = so[i] + pay;
        dof[i + 1] = dof[i] + pay;
        mo[i + 1] = mo[i] + HDR + HGH + pay;
    }
    const size_t src_bytes = so[NMSG], total = mo[NMSG], dst_bytes = dof[NMSG];
    uint8_t *src = malloc(src_bytes + 64);
    for (size_t k = 0; k < src_bytes + 64; k++)
        src[k] = (uint8_t) next_u64();

    void *d_src = NULL, *d_so = NULL, *d_buf = NULL, *d_mo = NULL, *d_dst = NULL, *d_do = NULL, *d_st = NULL,
         *d_cnt = NULL;
    const size_t tab = (NMSG + 1) * sizeof(uint64_t);
    hipStream_t s;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    HIPCHK(hipMalloc(&d_src, src_bytes + 64));
    HIPCHK(hipMalloc(&d_buf, total + 16));
    HIPCHK(hipMalloc(&d_dst, dst_bytes));
    HIPCHK(hipMalloc(&d_so, tab));
    HIPCHK(hipMalloc(&d_mo, tab));
    HIPCHK(hipMalloc(&d_do, tab));
    HIPCHK(hipMalloc(&d_st, NMSG));
    HIPCHK(hipMalloc(&d_cnt, sizeof(uint32_t)));
    HIPCHK(hipMemcpyAsync(d_src, src, src_bytes + 64, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_so, so, tab, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_mo, mo, tab, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_do, dof, tab, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_buf, 0xEE, total + 16, s));
    if (mchecksum_gpu_prepare("crc32c") != MCHECKSUM_GPU_OK) {
        fprintf(stderr, "prepare: %s\n", mchecksum_gpu_last_error());
        return 5;
    }
    /* the sender: payloads and hashes into the receive buffer */
    HIPCHK(hipMemsetAsync(d_st, 1, NMSG, s));
    int rc = mchecksum_gpu_pack_messages("crc32c", d_src, d_so, d_buf, d_mo, NMSG, HDR + HGH, HDR, d_st, s);
    if (rc != MCHECKSUM_GPU_OK) {
        fprintf(stderr, "pack_messages rc %d: %s\n", rc, mchecksum_gpu_last_error());
        return 6;
    }
    uint8_t *st = malloc(NMSG), *got = malloc(dst_bytes ? dst_bytes : 1);
    HIPCHK(hipMemcpyAsync(st, d_st, NMSG, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < NMSG; i++)
        if (st[i]) {
            fprintf(stderr, "pack_messages flagged message %zu\n", i);
            return 7;
        }

    const size_t flip_at = (size_t) mo[FLIP] + HDR + HGH + 57; /* a payload byte of message FLIP */
    for (int pass = 0; pass < 2; pass++) {
        uint32_t cnt = 0;
        if (pass == 1) { /* one payload bit flipped in the receive buffer */
            uint8_t b;
            HIPCHK(hipMemcpyAsync(&b, (uint8_t *) d_buf + flip_at, 1, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            b ^= 0x10;
            HIPCHK(hipMemcpyAsync((uint8_t *) d_buf + flip_at, &b, 1, hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
            src[so[FLIP] + 57] ^= 0x10; /* what the receiver must now see */
        }
        HIPCHK(hipMemsetAsync(d_dst, 0xEE, dst_bytes, s));
        HIPCHK(hipMemsetAsync(d_st, 1, NMSG, s));
        HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t), s));
        rc = mchecksum_gpu_unpack_messages("crc32c", d_buf, d_mo, NMSG, HDR + HGH, HDR, d_dst, d_do, d_st, d_cnt, s);
        if (rc != MCHECKSUM_GPU_OK) {
            fprintf(stderr, "unpack_messages rc %d: %s\n", rc, mchecksum_gpu_last_error());
            return 8;
        }
        HIPCHK(hipMemcpyAsync(got, d_dst, dst_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(st, d_st, NMSG, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        size_t bad_bytes = 0, wrong_status = 0, lead = 0;
        for (size_t k = 0; k < dof[0]; k++)
            lead += got[k] != 0xEE;
        for (size_t i = 0; i < NMSG; i++) {
            bad_bytes += memcmp(got + dof[i], src + so[i], so[i + 1] - so[i]) != 0;
            wrong_status += st[i] != (pass == 1 && i == FLIP ? 1 : 0);
        }
        printf("gpu receiver, %s: %d messages (%zu bytes) unpacked on a hipStream_t: payloads %zu differ, statuses %zu "
               "wrong, mismatches %u, bytes before the first payload changed %zu\n",
               pass ? "one payload bit flipped" : "as sent", NMSG, total, bad_bytes, wrong_status, cnt, lead);
        if (bad_bytes || wrong_status || lead || cnt != (uint32_t) pass)
            return 10 + pass;
    }
    HIPCHK(hipFree(d_src));
    HIPCHK(hipFree(d_buf));
    HIPCHK(hipFree(d_dst));
    HIPCHK(hipFree(d_so));
    HIPCHK(hipFree(d_mo));
    HIPCHK(hipFree(d_do));
    HIPCHK(hipFree(d_st));
    HIPCHK(hipFree(d_cnt));
    HIPCHK(hipStreamDestroy(s));
    printf("OK\n");
    return 0;
}
