// Internal face of the device JPEG decoder (csrc/jpeg_dev.hip) for the device readers in csrc/ingest.hip: a frame takes one
// staging slot for its depth and its colour.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct dms_jpeg_dev;

namespace dms {
namespace jpegdev {

struct FrameSlot {
  int index = -1;
  unsigned short* depth = nullptr;  // pinned, width * height
  unsigned char* rgb = nullptr;     // pinned, width * height * 3
};

int width(const dms_jpeg_dev* jd);
int height(const dms_jpeg_dev* jd);
int entropy_on_host(const dms_jpeg_dev* jd);
// takes the next slot of the ring (blocks while it is still in flight) and orders `stream` behind the object's last decode
int acquire(dms_jpeg_dev* jd, hipStream_t stream, FrameSlot* slot);
// JPEG -> rgb_dev through the slot; `who` prefixes the refusal text
int decode(dms_jpeg_dev* jd, const FrameSlot& slot, const unsigned char* data, size_t len, int flip, int on_host, void* rgb_dev,
           hipStream_t stream, const char* who);
// marks the slot in flight until everything enqueued on `stream` so far is done
int release(dms_jpeg_dev* jd, const FrameSlot& slot, hipStream_t stream);

}  // namespace jpegdev
}  // namespace dms
