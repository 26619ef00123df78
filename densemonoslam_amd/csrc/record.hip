// Recording: the writers' side of the ingest formats (include/dmslam_io.h), host code.  The readers are csrc/ingest.hip.
//   JPEG colour      csrc/jpeg_enc.hpp, libjpeg's bytes; what cvEncodeImage(".jpg", quality 90) gives the reference's converters
//                    (logs/rgbd/KlgToLcm.cpp:26-40, FreiburgLcm.cpp:24-38)
//   zlib depth       compress2 at the default level (KlgToLcm.cpp:111-145), resolved at run time as ingest.hip resolves uncompress
//   .klg             logs/rgbd/RawLogReader.cpp:30,70-110
//   LCM event log    the published eventlog layout (see ingest.hip)
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dmslam_io.h"
#include "common.hpp"
#include "deflate.hpp"
#include "jpeg_enc.hpp"

namespace {

typedef int (*compress2_fn)(unsigned char*, unsigned long*, const unsigned char*, unsigned long, int);
compress2_fn zlib_compress2() {
  static compress2_fn fn = [] {
    void* h = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libz.so", RTLD_NOW | RTLD_LOCAL);
    return h ? (compress2_fn)dlsym(h, "compress2") : (compress2_fn) nullptr;
  }();
  return fn;
}

inline void put_be32(unsigned char* p, uint32_t v) {
  p[0] = (unsigned char)(v >> 24);
  p[1] = (unsigned char)(v >> 16);
  p[2] = (unsigned char)(v >> 8);
  p[3] = (unsigned char)v;
}
inline void put_be64(unsigned char* p, uint64_t v) {
  put_be32(p, (uint32_t)(v >> 32));
  put_be32(p + 4, (uint32_t)v);
}

bool encode_args_ok(const char* who, int width, int height, int quality, int subsampling) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535) {
    dms::set_error("%s: image size %dx%d outside 1x1 .. 65535x65535", who, width, height);
    return false;
  }
  if (quality < 1 || quality > 100) {
    dms::set_error("%s: quality %d outside 1 .. 100", who, quality);
    return false;
  }
  if (subsampling != DMS_JPEG_420 && subsampling != DMS_JPEG_444) {
    dms::set_error("%s: subsampling %d is neither DMS_JPEG_420 nor DMS_JPEG_444", who, subsampling);
    return false;
  }
  return true;
}

}  // namespace

struct dms_klg_writer {
  FILE* fp = nullptr;
  int32_t frames = 0;
};

struct dms_lcmlog_writer {
  FILE* fp = nullptr;
  int64_t events = 0;
};

extern "C" {

size_t dms_jpeg_encode_bound(int width, int height, int subsampling) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || (subsampling != DMS_JPEG_420 && subsampling != DMS_JPEG_444)) return 0;
  return dms::jpeg::encode_bound(width, height, subsampling);
}

int dms_jpeg_encode(const unsigned char* rgb_host, int width, int height, int quality, int subsampling, int flipColors, void* out, size_t cap,
                    size_t* written) {
  DMS_REQUIRE(rgb_host && out && written, "null argument");
  if (!encode_args_ok("dms_jpeg_encode", width, height, quality, subsampling)) return DMS_ERR_INVALID_ARG;
  const size_t bound = dms::jpeg::encode_bound(width, height, subsampling);
  if (cap < bound) {
    *written = bound;
    dms::set_error("dms_jpeg_encode: buffer of %zu bytes, %zu needed for the worst case of %dx%d", cap, bound, width, height);
    return DMS_ERR_CAPACITY;
  }
  *written = dms::jpeg::encode_rgb(rgb_host, width, height, quality, subsampling, flipColors ? 1 : 0, (unsigned char*)out);
  return DMS_OK;
}

size_t dms_deflate_bound(size_t len) { return len + (len >> 12) + (len >> 14) + (len >> 25) + 13 + 64; }  // compressBound, with room

int dms_deflate(const void* data, size_t len, void* out, size_t cap, size_t* written) {
  DMS_REQUIRE(data && out && written, "null argument");
  compress2_fn c2 = zlib_compress2();
  if (!c2) {
    dms::set_error("zlib (libz.so.1) is not loadable: depth cannot be compressed");
    return DMS_ERR_UNSUPPORTED;
  }
  if (cap < dms_deflate_bound(len)) {
    *written = dms_deflate_bound(len);
    dms::set_error("dms_deflate: buffer of %zu bytes, %zu needed", cap, *written);
    return DMS_ERR_CAPACITY;
  }
  unsigned long n = (unsigned long)cap;
  const int rc = c2((unsigned char*)out, &n, (const unsigned char*)data, (unsigned long)len, -1 /* Z_DEFAULT_COMPRESSION */);
  if (rc != 0) {
    dms::set_error("zlib compress2 failed (rc %d)", rc);
    return DMS_ERR_FORMAT;
  }
  *written = (size_t)n;
  return DMS_OK;
}

size_t dms_deflate_blocks_block_size(void) { return dms::dfl::kBlock; }
size_t dms_deflate_blocks_bound(size_t len) { return dms::dfl::stream_bound(len); }

int dms_deflate_blocks(const void* data, size_t len, void* out, size_t cap, size_t* written) {
  DMS_REQUIRE(data && out && written, "null argument");
  DMS_REQUIRE(len >= 1 && len <= ((size_t)1 << 31), "len outside 1 .. 2^31");
  if (cap < dms::dfl::stream_bound(len)) {
    *written = dms::dfl::stream_bound(len);
    dms::set_error("dms_deflate_blocks: buffer of %zu bytes, %zu needed", cap, *written);
    return DMS_ERR_CAPACITY;
  }
  *written = dms::dfl::encode((const unsigned char*)data, len, (unsigned char*)out);
  return DMS_OK;
}

int dms_frame_pack(const unsigned short* depth_host, const unsigned char* rgb_host, int width, int height, int compressed, int quality, int flipColors,
                   int64_t timestamp, int32_t frameNumber, const char* senderName, dms_frame_msg* m, void** owned) {
  DMS_REQUIRE(depth_host && rgb_host && m && owned, "null argument");
  DMS_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "bad image size");
  DMS_REQUIRE(compressed || !flipColors, "a raw frame is not copied: flipColors needs compressed = 1");
  const size_t px = (size_t)width * height;
  DMS_REQUIRE(px * 3 <= 0x7fffffffu, "a frame of more than 2 GiB");
  *owned = nullptr;
  memset(m, 0, sizeof(*m));
  m->compressed = compressed ? 1 : 0;
  m->timestamp = timestamp;
  m->frameNumber = frameNumber;
  if (senderName) {
    strncpy(m->senderName, senderName, sizeof(m->senderName) - 1);
  }
  if (!compressed) {
    m->depth = (const unsigned char*)depth_host;
    m->depthSize = (int32_t)(px * 2);
    m->image = rgb_host;
    m->imageSize = (int32_t)(px * 3);
    return DMS_OK;
  }
  if (!encode_args_ok("dms_frame_pack", width, height, quality, DMS_JPEG_420)) return DMS_ERR_INVALID_ARG;
  const size_t dcap = dms_deflate_bound(px * 2), icap = dms::jpeg::encode_bound(width, height, DMS_JPEG_420);
  unsigned char* buf = (unsigned char*)malloc(dcap + icap);
  if (!buf) {
    dms::set_error("dms_frame_pack: out of memory");
    return DMS_ERR_WORKSPACE;
  }
  size_t dn = 0, in = 0;
  int rc = dms_deflate(depth_host, px * 2, buf, dcap, &dn);
  if (!rc) rc = dms_jpeg_encode(rgb_host, width, height, quality, DMS_JPEG_420, flipColors, buf + dcap, icap, &in);
  if (rc) {
    free(buf);
    return rc;
  }
  m->depth = buf;
  m->depthSize = (int32_t)dn;
  m->image = buf + dcap;
  m->imageSize = (int32_t)in;
  *owned = buf;
  return DMS_OK;
}

void dms_frame_pack_free(void* owned) { free(owned); }

int dms_klg_writer_open(dms_klg_writer** out, const char* path) {
  DMS_REQUIRE(out && path, "null argument");
  FILE* fp = fopen(path, "wb");
  const int32_t zero = 0;
  if (!fp || fwrite(&zero, sizeof(zero), 1, fp) != 1) {
    if (fp) fclose(fp);
    dms::set_error("dms_klg_writer_open: cannot write %s", path);
    return DMS_ERR_INVALID_ARG;
  }
  dms_klg_writer* w = new dms_klg_writer();
  w->fp = fp;
  *out = w;
  return DMS_OK;
}

int dms_klg_writer_append(dms_klg_writer* w, int64_t timestamp, const void* depth_bytes, int32_t depthSize, const void* image_bytes, int32_t imageSize) {
  DMS_REQUIRE(w && w->fp, "null argument");
  DMS_REQUIRE(depthSize > 0 && depth_bytes && imageSize >= 0 && (imageSize == 0 || image_bytes), "bad payload");
  if (fwrite(&timestamp, sizeof(timestamp), 1, w->fp) != 1 || fwrite(&depthSize, sizeof(depthSize), 1, w->fp) != 1 ||
      fwrite(&imageSize, sizeof(imageSize), 1, w->fp) != 1 || fwrite(depth_bytes, 1, (size_t)depthSize, w->fp) != (size_t)depthSize ||
      (imageSize && fwrite(image_bytes, 1, (size_t)imageSize, w->fp) != (size_t)imageSize)) {
    dms::set_error("dms_klg_writer_append: write failed");
    return DMS_ERR_STATE;
  }
  ++w->frames;
  return DMS_OK;
}

int dms_klg_writer_close(dms_klg_writer* w) {
  if (!w) return DMS_OK;
  int rc = DMS_OK;
  if (w->fp) {
    if (fseek(w->fp, 0, SEEK_SET) != 0 || fwrite(&w->frames, sizeof(w->frames), 1, w->fp) != 1) rc = DMS_ERR_STATE;
    if (fclose(w->fp) != 0) rc = DMS_ERR_STATE;
    if (rc) dms::set_error("dms_klg_writer_close: the frame count could not be written");
  }
  delete w;
  return rc;
}

int dms_lcmlog_writer_open(dms_lcmlog_writer** out, const char* path) {
  DMS_REQUIRE(out && path, "null argument");
  FILE* fp = fopen(path, "wb");
  if (!fp) {
    dms::set_error("dms_lcmlog_writer_open: cannot write %s", path);
    return DMS_ERR_INVALID_ARG;
  }
  dms_lcmlog_writer* w = new dms_lcmlog_writer();
  w->fp = fp;
  *out = w;
  return DMS_OK;
}

int dms_lcmlog_writer_append(dms_lcmlog_writer* w, int64_t timestamp_us, const char* channel, const void* data, size_t len) {
  DMS_REQUIRE(w && w->fp && channel && (data || !len), "null argument");
  const size_t cl = strlen(channel);
  DMS_REQUIRE(cl <= 65536 && len <= ((size_t)1 << 30), "channel or data longer than the reader accepts");
  unsigned char hdr[28];
  put_be32(hdr, 0xEDA1DA01u);
  put_be64(hdr + 4, (uint64_t)w->events);
  put_be64(hdr + 12, (uint64_t)timestamp_us);
  put_be32(hdr + 20, (uint32_t)cl);
  put_be32(hdr + 24, (uint32_t)len);
  if (fwrite(hdr, 1, sizeof(hdr), w->fp) != sizeof(hdr) || (cl && fwrite(channel, 1, cl, w->fp) != cl) || (len && fwrite(data, 1, len, w->fp) != len)) {
    dms::set_error("dms_lcmlog_writer_append: write failed");
    return DMS_ERR_STATE;
  }
  ++w->events;
  return DMS_OK;
}

int dms_lcmlog_writer_close(dms_lcmlog_writer* w) {
  if (!w) return DMS_OK;
  int rc = DMS_OK;
  if (w->fp && fclose(w->fp) != 0) {
    dms::set_error("dms_lcmlog_writer_close: close failed");
    rc = DMS_ERR_STATE;
  }
  delete w;
  return rc;
}

}  // extern "C"
