// crc_gpu_device.h -- device side of the MI355X (gfx950) batch CRC kernels:
// the table-driven step loops, sub-stream combine trees and the persistent
// batch kernels.  Included by the translation units that launch them
// (mchecksum_gpu.hip: fixed / offsets / verify batches; mchecksum_gpu_ext.hip:
// scatter-gather segments and core headers).  Algebra: crc_gpu_layout.h.
//
// An umbrella: the parts, in the order they build on each other.  The first
// three are plain C++ that the host's launch plan and the CPU tests compile
// too.
#ifndef CRC_GPU_DEVICE_H
#define CRC_GPU_DEVICE_H

#include "crc_gpu_shape.h"   // launch shapes, LDS maps, BatchArgs, queue layout
#include "crc_gpu_plan.h"    // the work queue's chunk plan
#include "crc_gpu_window.h"  // payload window geometry
#include "crc_gpu_queue.h"   // work-queue protocol, bounded waits, trace stamps
#include "crc_gpu_common.h"  // loads, emit, mismatch count: shared by both widths
#include "crc_gpu_crc32.h"   // CRC-32C fold, combine, payload loops, batch kernel
#include "crc_gpu_crc64.h"   // CRC-64 likewise

#endif  // CRC_GPU_DEVICE_H
