// What csrc/jpeg_enc_dev.hip needs of csrc/deflate_dev.hip beyond include/dmslam_io_write.h: an encode into a pinned area of the
// caller's (the JPEG encoder's slot) through slot `index` of the deflate object's ring.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dmslam_io_write.h"
#include "deflate_core.hpp"

namespace dms {
namespace dfl {

// bytes of a pinned area for input of `len` bytes: [length word (16 bytes) | stream]
size_t dev_slot_bytes(size_t len);
// everything of one encode onto `stream`; the arguments are checked, the slot is free.  *eager: the bytes of the stream copied here
int dev_enqueue(dms_deflate_dev* dd, int index, const void* data_dev, size_t len, hipStream_t stream, unsigned char* pinned, size_t* eager);
// after the work enqueued above is done: copies what is left of the stream and hands it out
int dev_finish(dms_deflate_dev* dd, int index, unsigned char* pinned, size_t eager, const unsigned char** data, size_t* len);

}  // namespace dfl
}  // namespace dms
