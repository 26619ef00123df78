/* dmslam_io.h — frame ingest formats either side of the hot path.
 *
 * Replaces, for a maintainer wiring real datasets into the back end:
 *   - eflcm::Frame, the LCM message every live / logged camera publishes
 *       (logs/rgbd/eflcm/Frame.py:27-65, logs/rgbd/lcmtypes, GUI/src/Tools/LcmHandler.h);
 *   - RawLcmLogReader (GUI/src/Tools/RawLcmLogReader.h:37-85): LCM event log -> frames;
 *   - RawLogReader / .klg (logs/rgbd/RawLogReader.cpp:30,70-110).
 * Host-side, plain C ABI, no device work: the decoded depth (u16 mm) and RGB8 buffers are what
 * dms_memcpy_h2d + dms_fusion_process_frame take.  zlib (depth) is loaded at run time; JPEG colour is
 * decoded by the library's own baseline decoder (csrc/jpeg.hpp: libjpeg's default arithmetic — slow integer
 * inverse DCT, fancy upsampling, fixed-point colour conversion — byte for byte; progressive / arithmetic-coded /
 * non-YCbCr streams return DMS_ERR_UNSUPPORTED).
 */
#ifndef DMSLAM_IO_H_
#define DMSLAM_IO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef DMS_ERR_UNSUPPORTED
#define DMS_ERR_UNSUPPORTED (-7) /* e.g. a progressive JPEG, or zlib not loadable */
#endif
#define DMS_ERR_FORMAT (-8)      /* malformed message / log */
#ifndef DMS_ERR_CAPACITY
#define DMS_ERR_CAPACITY (-4)    /* an output buffer is too small (dmslam.h) */
#endif
#define DMS_EOF 1                /* readers: no more frames (not an error) */

/* eflcm::Frame with `depth` / `image` as views into the encoded message (decode) or caller
 * buffers (encode).  Wire layout (big-endian): 8-byte fingerprint 9f620b14f1894896, then
 * b trackOnly, b compressed, b last, i32 depthSize, i32 imageSize, depth bytes, image bytes,
 * i64 timestamp, i32 frameNumber, u32 len(senderName)+1, senderName, NUL (Frame.py:33-41). */
typedef struct dms_frame_msg {
  int trackOnly, compressed, last;
  int32_t depthSize, imageSize;
  const unsigned char* depth;
  const unsigned char* image;
  int64_t timestamp;
  int32_t frameNumber;
  char senderName[128];
} dms_frame_msg;

size_t dms_eflcm_frame_encoded_size(const dms_frame_msg* m);
int dms_eflcm_frame_encode(const dms_frame_msg* m, void* buf, size_t cap, size_t* written);
int dms_eflcm_frame_decode(const void* data, size_t len, dms_frame_msg* out);

/* Baseline JPEG -> W*H*3 bytes in libjpeg's R, G, B scanline order: what jpeg_read_scanlines hands
 * JPEGLoader::readData (GUI/src/Tools/JPEGLoader.h:44-95) before its per-pixel R<->B exchange.  The size
 * in the stream must equal width x height. */
int dms_jpeg_decode(const void* data, size_t len, int width, int height, unsigned char* rgb_out);

/* message -> W*H u16 depth + W*H*3 RGB8, as RawLcmLogReader::getNext does (uncompress / copy,
 * optional R<->B swap) */
int dms_frame_unpack(const dms_frame_msg* m, int width, int height, int flipColors, unsigned short* depth_out,
                     unsigned char* rgb_out);

/* LCM event log (lcm::LogFile): events of {sync 0xEDA1DA01, i64 eventnum, i64 timestamp_us,
 * i32 channel length, i32 data length, channel, data}, big-endian */
typedef struct dms_lcmlog dms_lcmlog;
int dms_lcmlog_open(dms_lcmlog** out, const char* path);
/* next event; `data` stays valid until the next call.  Returns DMS_EOF at the end. */
int dms_lcmlog_next(dms_lcmlog* h, char* channel, size_t channel_cap, const void** data, size_t* len, int64_t* timestamp_us);
int dms_lcmlog_rewind(dms_lcmlog* h);
int dms_lcmlog_close(dms_lcmlog* h);

/* .klg: i32 numFrames, then per frame i64 timestamp, i32 depthSize, i32 imageSize, depth, image
 * (little-endian; raw when the sizes equal W*H*2 / W*H*3, zlib depth / JPEG colour otherwise;
 * imageSize 0 = black image) */
typedef struct dms_klg dms_klg;
int dms_klg_open(dms_klg** out, const char* path, int width, int height, int flipColors);
int dms_klg_num_frames(dms_klg* h);
int dms_klg_next(dms_klg* h, unsigned short* depth_out, unsigned char* rgb_out, int64_t* timestamp);
int dms_klg_rewind(dms_klg* h);
int dms_klg_close(dms_klg* h);

/* ---- recording: the writers' side of the formats above (csrc/record.hip; the device forms are in dmslam_io_write.h) ----
 *
 * RGB8 (libjpeg's R, G, B order; R and B exchanged on the way in where flipColors) -> a baseline JPEG file, SOI to EOI, the
 * bytes libjpeg's C encoder writes with its default parameters (csrc/jpeg_enc.hpp: fixed-point colour conversion, h2v2 box
 * filter, slow integer forward DCT, jpeg_set_quality(quality, force_baseline) tables, the standard Huffman tables, JFIF 1.01
 * header; sequential, 8 bit, three components, no restart markers, no optimised tables).  What the reference's converters
 * write with cvEncodeImage(".jpg", quality 90) (logs/rgbd/KlgToLcm.cpp:26-40).
 * quality 1..100; subsampling DMS_JPEG_420 (libjpeg's and OpenCV's default) or DMS_JPEG_444; width, height 1..65535.
 * cap below dms_jpeg_encode_bound: DMS_ERR_CAPACITY (-4) and *written receives that bound. */
#define DMS_JPEG_444 0
#define DMS_JPEG_420 2
size_t dms_jpeg_encode_bound(int width, int height, int subsampling); /* the header + every block at its longest, stuffed; 0 = bad arguments */
int dms_jpeg_encode(const unsigned char* rgb_host, int width, int height, int quality, int subsampling, int flipColors,
                    void* out, size_t cap, size_t* written);

/* zlib's compress2 at its default level, as the reference's converters deflate depth (KlgToLcm.cpp:111-145); libz.so.1 is
 * resolved at run time: DMS_ERR_UNSUPPORTED where it is not loadable.  cap below dms_deflate_bound: DMS_ERR_CAPACITY. */
size_t dms_deflate_bound(size_t len);
int dms_deflate(const void* data, size_t len, void* out, size_t cap, size_t* written);

/* A zlib stream of independent-to-make deflate blocks (csrc/deflate_core.hpp: a block per 4096 input bytes, each the cheapest of
 * stored, fixed and dynamic Huffman, matches reaching back into earlier blocks' input), the bytes dms_deflate_dev (dmslam_io_write.h)
 * writes on the device; no libz needed.  Any inflate reads it.  len == 0 or above 2^31: DMS_ERR_INVALID_ARG; cap below
 * dms_deflate_blocks_bound(len): DMS_ERR_CAPACITY with the bound in *written. */
size_t dms_deflate_blocks_block_size(void);
size_t dms_deflate_blocks_bound(size_t len);
int dms_deflate_blocks(const void* data, size_t len, void* out, size_t cap, size_t* written);

/* One frame -> an eflcm::Frame ready for dms_eflcm_frame_encode.  compressed = 0: m->depth / m->image are the caller's
 * buffers (nothing is copied; flipColors must be 0).  compressed = 1: zlib depth and JPEG colour (quality, DMS_JPEG_420) in
 * a buffer the message owns; release it with dms_frame_pack_free (a no-op for raw messages and zeroed structs). */
int dms_frame_pack(const unsigned short* depth_host, const unsigned char* rgb_host, int width, int height, int compressed, int quality,
                   int flipColors, int64_t timestamp, int32_t frameNumber, const char* senderName, dms_frame_msg* m, void** owned);
void dms_frame_pack_free(void* owned);

/* .klg writer: the count is written as 0 at open and rewritten at close.  The payloads are the frame's bytes as they go into
 * the file (raw or compressed; imageSize 0 = no image). */
typedef struct dms_klg_writer dms_klg_writer;
int dms_klg_writer_open(dms_klg_writer** out, const char* path);
int dms_klg_writer_append(dms_klg_writer* w, int64_t timestamp, const void* depth_bytes, int32_t depthSize, const void* image_bytes,
                          int32_t imageSize);
int dms_klg_writer_close(dms_klg_writer* w);

/* LCM event log writer: events numbered from 0 in the order of the appends */
typedef struct dms_lcmlog_writer dms_lcmlog_writer;
int dms_lcmlog_writer_open(dms_lcmlog_writer** out, const char* path);
int dms_lcmlog_writer_append(dms_lcmlog_writer* w, int64_t timestamp_us, const char* channel, const void* data, size_t len);
int dms_lcmlog_writer_close(dms_lcmlog_writer* w);

#ifdef __cplusplus
}
#endif
#endif /* DMSLAM_IO_H_ */
