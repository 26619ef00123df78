/* Test infrastructure: the GL host of tests/golden/make_ref_render_cloud_golden.py (which compiles it into a temporary directory).
 *
 * Runs the REFERENCE's own feedback programs - vertex_feedback.{vert,geom} and draw_feedback.{vert,frag}, read at RUN time from the
 * shader directory given on the command line (never copied into this repository) - on Mesa's llvmpipe, with the call sequences of
 * FeedbackBuffer::compute and FeedbackBuffer::render (Core/src/Shaders/FeedbackBuffer.cpp:84-187) as GUI/src/MainController.cpp:475-493
 * issues them, and the GUI's framebuffer state: RGBA8 colour, DEPTH_COMPONENT24, depth test on, GL_LESS, point size 1.  The context is
 * made as tests/golden/gl_render_host.c makes it.  The textures are the context's (Context.h:158-177): the colour image and the raw
 * metric depth LINEAR, the filtered metric depth NEAREST, CLAMP_TO_EDGE.  NUM_CAMERAS comes from the reference's size.glsl: the vertex
 * is 60 bytes (position, colour, three times, normal).
 *
 *   gl_render_cloud_host SHADER_DIR REQUEST OUTPUT
 * REQUEST (little endian): int32 W, H, cols, rows, n_draws; float32 clear_rgba[4], fx, fy, cx, cy, maxDepth; cols*rows RGBA8;
 * cols*rows float32 raw metric depth; cols*rows float32 filtered metric depth (image rows, top first); per draw: int32 buffer (0 RAW,
 * 1 FILTERED), colorType; float32 mvp[16], pose[16] (row-major).  Both buffers are computed once; all draws go into one framebuffer.
 * OUTPUT: W*H RGBA8 (glReadPixels, rows bottom-up), W*H uint32 24-bit depth, then int32 vertex counts of the RAW and FILTERED buffer
 * (GL_TRANSFORM_FEEDBACK_PRIMITIVES_WRITTEN of each feedback pass).
 */
#include <GL/gl.h>
#include <GL/glext.h>
#include <GL/internal/dri_interface.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define GLFUNCS(X)                                                                                                               \
  X(PFNGLCREATESHADERPROC, glCreateShader) X(PFNGLSHADERSOURCEPROC, glShaderSource) X(PFNGLCOMPILESHADERPROC, glCompileShader)   \
  X(PFNGLGETSHADERIVPROC, glGetShaderiv) X(PFNGLGETSHADERINFOLOGPROC, glGetShaderInfoLog) X(PFNGLCREATEPROGRAMPROC, glCreateProgram) \
  X(PFNGLATTACHSHADERPROC, glAttachShader) X(PFNGLLINKPROGRAMPROC, glLinkProgram) X(PFNGLGETPROGRAMIVPROC, glGetProgramiv)       \
  X(PFNGLGETPROGRAMINFOLOGPROC, glGetProgramInfoLog) X(PFNGLUSEPROGRAMPROC, glUseProgram)                                         \
  X(PFNGLGETUNIFORMLOCATIONPROC, glGetUniformLocation) X(PFNGLUNIFORM1IPROC, glUniform1i) X(PFNGLUNIFORM1FPROC, glUniform1f)       \
  X(PFNGLUNIFORM3FPROC, glUniform3f) X(PFNGLUNIFORMMATRIX4FVPROC, glUniformMatrix4fv) X(PFNGLGENBUFFERSPROC, glGenBuffers)         \
  X(PFNGLBINDBUFFERPROC, glBindBuffer) X(PFNGLBUFFERDATAPROC, glBufferData) X(PFNGLGENVERTEXARRAYSPROC, glGenVertexArrays)         \
  X(PFNGLBINDVERTEXARRAYPROC, glBindVertexArray) X(PFNGLENABLEVERTEXATTRIBARRAYPROC, glEnableVertexAttribArray)                   \
  X(PFNGLDISABLEVERTEXATTRIBARRAYPROC, glDisableVertexAttribArray) X(PFNGLVERTEXATTRIBPOINTERPROC, glVertexAttribPointer)         \
  X(PFNGLGENFRAMEBUFFERSPROC, glGenFramebuffers) X(PFNGLBINDFRAMEBUFFERPROC, glBindFramebuffer)                                   \
  X(PFNGLFRAMEBUFFERRENDERBUFFERPROC, glFramebufferRenderbuffer) X(PFNGLGENRENDERBUFFERSPROC, glGenRenderbuffers)                 \
  X(PFNGLBINDRENDERBUFFERPROC, glBindRenderbuffer) X(PFNGLRENDERBUFFERSTORAGEPROC, glRenderbufferStorage)                         \
  X(PFNGLCHECKFRAMEBUFFERSTATUSPROC, glCheckFramebufferStatus) X(PFNGLDRAWBUFFERSPROC, glDrawBuffers)                          \
  X(PFNGLTRANSFORMFEEDBACKVARYINGSPROC, glTransformFeedbackVaryings) X(PFNGLBINDBUFFERBASEPROC, glBindBufferBase)                \
  X(PFNGLBEGINTRANSFORMFEEDBACKPROC, glBeginTransformFeedback) X(PFNGLENDTRANSFORMFEEDBACKPROC, glEndTransformFeedback)          \
  X(PFNGLGENTRANSFORMFEEDBACKSPROC, glGenTransformFeedbacks) X(PFNGLBINDTRANSFORMFEEDBACKPROC, glBindTransformFeedback)          \
  X(PFNGLDRAWTRANSFORMFEEDBACKPROC, glDrawTransformFeedback) X(PFNGLUNIFORM4FPROC, glUniform4f)                                  \
  X(PFNGLGENQUERIESPROC, glGenQueries) X(PFNGLBEGINQUERYPROC, glBeginQuery) X(PFNGLENDQUERYPROC, glEndQuery)                       \
  X(PFNGLGETQUERYOBJECTUIVPROC, glGetQueryObjectuiv)
#define DECL(T, n) static T n;
GLFUNCS(DECL)
static void (*p_glViewport)(GLint, GLint, GLsizei, GLsizei);
static void (*p_glClearColor)(GLfloat, GLfloat, GLfloat, GLfloat);
static void (*p_glClear)(GLbitfield);
static void (*p_glEnable)(GLenum);
static void (*p_glDepthFunc)(GLenum);
static void (*p_glDepthMask)(GLboolean);
static void (*p_glDrawArrays)(GLenum, GLint, GLsizei);
static void (*p_glFinish)(void);
static GLenum (*p_glGetError)(void);
static void (*p_glPixelStorei)(GLenum, GLint);
static void (*p_glReadPixels)(GLint, GLint, GLsizei, GLsizei, GLenum, GLenum, void*);
static void (*p_glReadBuffer)(GLenum);
static void (*p_glPointSize)(GLfloat);
static void (*p_glDisable)(GLenum);
static void (*p_glActiveTexture)(GLenum);
static void (*p_glGenTextures)(GLsizei, GLuint*);
static void (*p_glBindTexture)(GLenum, GLuint);
static void (*p_glTexImage2D)(GLenum, GLint, GLint, GLsizei, GLsizei, GLint, GLenum, GLenum, const void*);
static void (*p_glTexParameteri)(GLenum, GLenum, GLint);

static char g_dir[1024];

static void die(const char* what, const char* detail) {
  fprintf(stderr, "gl_render_cloud_host: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
  exit(1);
}

static void getDrawableInfo(__DRIdrawable* d, int* x, int* y, int* w, int* h, void* p) { (void)d; (void)p; *x = *y = 0; *w = *h = 16; }
static void putImage(__DRIdrawable* d, int op, int x, int y, int w, int h, char* data, void* p) { (void)d; (void)op; (void)x; (void)y; (void)w; (void)h; (void)data; (void)p; }
static void getImage(__DRIdrawable* d, int x, int y, int w, int h, char* data, void* p) { (void)d; (void)x; (void)y; (void)w; (void)h; (void)data; (void)p; }
static const __DRIswrastLoaderExtension swrastLoader = {{__DRI_SWRAST_LOADER, 1}, getDrawableInfo, putImage, getImage};
static const __DRIextension* loader_ext[] = {&swrastLoader.base, NULL};

static void make_context(void) {
  const char* paths[] = {"/usr/lib/x86_64-linux-gnu/dri/swrast_dri.so", "swrast_dri.so", NULL};
  void* h = NULL;
  for (int i = 0; paths[i] && !h; i++) h = dlopen(paths[i], RTLD_NOW | RTLD_GLOBAL);
  if (!h) die("Mesa's swrast_dri.so not found", dlerror());
  const __DRIextension** (*get)(void) = (const __DRIextension** (*)(void))dlsym(h, "__driDriverGetExtensions_swrast");
  if (!get) die("__driDriverGetExtensions_swrast missing", NULL);
  const __DRIextension** ext = get();
  const __DRIcoreExtension* core = NULL;
  const __DRIswrastExtension* sw = NULL;
  for (int i = 0; ext[i]; i++) {
    if (!strcmp(ext[i]->name, __DRI_CORE)) core = (const __DRIcoreExtension*)ext[i];
    if (!strcmp(ext[i]->name, __DRI_SWRAST)) sw = (const __DRIswrastExtension*)ext[i];
  }
  if (!core || !sw || sw->base.version < 4) die("DRI_Core / DRI_SWRast (v4) not offered by the driver", NULL);
  const __DRIconfig** configs = NULL;
  __DRIscreen* scr = sw->createNewScreen2(0, loader_ext, ext, &configs, NULL);
  if (!scr || !configs || !configs[0]) die("createNewScreen2 failed", NULL);
  unsigned err = 0;
  uint32_t attribs[] = {__DRI_CTX_ATTRIB_MAJOR_VERSION, 4, __DRI_CTX_ATTRIB_MINOR_VERSION, 5};
  __DRIcontext* ctx = sw->createContextAttribs(scr, __DRI_API_OPENGL_CORE, configs[0], NULL, 2, attribs, &err, NULL);
  if (!ctx) die("no OpenGL 4.5 core context from llvmpipe", NULL);
  __DRIdrawable* dr = sw->createNewDrawable(scr, configs[0], NULL);
  if (!dr || !core->bindContext(ctx, dr, dr)) die("bindContext failed", NULL);
  void* glapi = dlopen("libglapi.so.0", RTLD_NOW | RTLD_GLOBAL);
  if (!glapi) die("libglapi.so.0 not found", dlerror());
  void* (*gpa)(const char*) = (void* (*)(const char*))dlsym(glapi, "_glapi_get_proc_address");
  if (!gpa) die("_glapi_get_proc_address missing", NULL);
#define LOAD(T, n) \
  n = (T)gpa(#n);  \
  if (!n) die("GL entry point missing", #n);
  GLFUNCS(LOAD)
#define LOAD1(n)               \
  *(void**)(&p_##n) = gpa(#n); \
  if (!p_##n) die("GL entry point missing", #n);
  LOAD1(glViewport) LOAD1(glClearColor) LOAD1(glClear) LOAD1(glEnable) LOAD1(glDepthFunc) LOAD1(glDepthMask) LOAD1(glDrawArrays)
  LOAD1(glFinish) LOAD1(glGetError) LOAD1(glPixelStorei) LOAD1(glReadPixels) LOAD1(glReadBuffer) LOAD1(glPointSize)
  LOAD1(glDisable) LOAD1(glActiveTexture) LOAD1(glGenTextures) LOAD1(glBindTexture) LOAD1(glTexImage2D) LOAD1(glTexParameteri)
}

/* shader files where they lie, `#include "x"` expanded by textual insertion as Pangolin does */
static char* read_file(const char* name) {
  char path[1400];
  snprintf(path, sizeof path, "%s/%s", g_dir, name);
  FILE* f = fopen(path, "rb");
  if (!f) die("cannot read shader", path);
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  char* s = (char*)malloc(n + 1);
  if (fread(s, 1, n, f) != (size_t)n) die("short read", path);
  s[n] = 0;
  fclose(f);
  return s;
}
static char* expand(const char* name, int depth) {
  char* src = read_file(name);
  if (depth > 4) return src;
  size_t cap = strlen(src) + 1, len = 0;
  char* out = (char*)malloc(cap);
  out[0] = 0;
  for (char* line = src; *line;) {
    char* nl = strchr(line, '\n');
    size_t ll = nl ? (size_t)(nl - line) + 1 : strlen(line);
    char inc[256], one[512];
    char* piece = NULL;
    size_t cl = ll < sizeof one - 1 ? ll : sizeof one - 1;
    memcpy(one, line, cl);
    one[cl] = 0;
    if (sscanf(one, " #include \"%255[^\"]\"", inc) == 1) piece = expand(inc, depth + 1);
    size_t pl = piece ? strlen(piece) + 1 : ll;
    if (len + pl + 1 > cap) {
      cap = (len + pl + 1) * 2;
      out = (char*)realloc(out, cap);
    }
    if (piece) {
      memcpy(out + len, piece, pl - 1);
      out[len + pl - 1] = '\n';
      free(piece);
    } else {
      memcpy(out + len, line, ll);
    }
    len += pl;
    out[len] = 0;
    line += ll;
  }
  free(src);
  return out;
}
static GLuint compile(GLenum type, const char* name) {
  char* src = expand(name, 0);
  GLuint s = glCreateShader(type);
  const char* p = src;
  glShaderSource(s, 1, &p, NULL);
  glCompileShader(s);
  GLint ok = 0;
  glGetShaderiv(s, GL_COMPILE_STATUS, &ok);
  free(src);
  if (!ok) {
    char log[3000];
    glGetShaderInfoLog(s, sizeof log, NULL, log);
    die(name, log);
  }
  return s;
}
/* loadProgramGeomFromFile / loadProgramFromFile (Shaders/Shaders.h); tf: the four interleaved feedback varyings, named before
 * linking (core GL) where FeedbackBuffer.cpp:57-66 names them through the NV extension afterwards */
static GLuint program(const char* vs, const char* gs, const char* fs, int tf) {
  static const char* TF4[] = {"vPosition0", "vColor0", "vTimes0", "vNormRad0"};
  GLuint p = glCreateProgram();
  glAttachShader(p, compile(GL_VERTEX_SHADER, vs));
  if (gs) glAttachShader(p, compile(GL_GEOMETRY_SHADER, gs));
  if (fs) glAttachShader(p, compile(GL_FRAGMENT_SHADER, fs));
  if (tf) glTransformFeedbackVaryings(p, 4, TF4, GL_INTERLEAVED_ATTRIBS);
  glLinkProgram(p);
  GLint ok = 0;
  glGetProgramiv(p, GL_LINK_STATUS, &ok);
  if (!ok) {
    char log[3000];
    glGetProgramInfoLog(p, sizeof log, NULL, log);
    die(vs, log);
  }
  return p;
}
/* Uniform MAT4: Eigen / pangolin storage is column-major; the request is row-major */
static void um4(GLuint p, const char* n, const float* rowmajor) {
  float cm[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) cm[c * 4 + r] = rowmajor[r * 4 + c];
  glUniformMatrix4fv(glGetUniformLocation(p, n), 1, GL_FALSE, cm);
}

static void rd(void* dst, size_t bytes, FILE* f) {
  if (fread(dst, 1, bytes, f) != bytes) die("short request", NULL);
}

static GLuint tex2d(int w, int h, GLint ifmt, GLenum fmt, GLenum type, const void* data, int linear) {
  GLuint t;
  p_glGenTextures(1, &t);
  p_glBindTexture(GL_TEXTURE_2D, t);
  p_glPixelStorei(GL_UNPACK_ALIGNMENT, 1);
  p_glTexImage2D(GL_TEXTURE_2D, 0, ifmt, w, h, 0, fmt, type, data);
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MIN_FILTER, linear ? GL_LINEAR : GL_NEAREST); /* pangolin::GlTexture::Reinitialise */
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MAG_FILTER, linear ? GL_LINEAR : GL_NEAREST);
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_WRAP_S, GL_CLAMP_TO_EDGE);
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_WRAP_T, GL_CLAMP_TO_EDGE);
  return t;
}

#define VERTEX_BYTES 60

int main(int argc, char** argv) {
  if (argc != 4) die("usage: gl_render_cloud_host SHADER_DIR REQUEST OUTPUT", NULL);
  snprintf(g_dir, sizeof g_dir, "%s", argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) die("cannot open request", argv[2]);
  int32_t hdr[5];
  float fl[9];
  rd(hdr, sizeof hdr, f);
  rd(fl, sizeof fl, f);
  const int W = hdr[0], H = hdr[1], cols = hdr[2], rows = hdr[3], nd = hdr[4];
  const size_t np = (size_t)cols * rows;
  uint8_t* img = (uint8_t*)malloc(np * 4);
  float* dm[2] = {(float*)malloc(np * 4), (float*)malloc(np * 4)};
  rd(img, np * 4, f);
  rd(dm[0], np * 4, f);
  rd(dm[1], np * 4, f);

  make_context();
  GLuint vao;
  glGenVertexArrays(1, &vao);
  glBindVertexArray(vao);
  const GLuint feedback_prog = program("vertex_feedback.vert", "vertex_feedback.geom", NULL, 1);
  const GLuint draw_prog = program("draw_feedback.vert", NULL, "draw_feedback.frag", 0);

  /* FeedbackBuffer::FeedbackBuffer (:22-74): the uv buffer in column-major pixel order, in the constructor's arithmetic */
  float* uv = (float*)malloc(np * 8);
  for (int i = 0, k = 0; i < cols; i++)
    for (int j = 0; j < rows; j++, k++) {
      uv[2 * k] = (float)(((float)i / (float)cols) + 1.0 / (2 * (float)cols));
      uv[2 * k + 1] = (float)(((float)j / (float)rows) + 1.0 / (2 * (float)rows));
    }
  GLuint uvo, vbo[2], fid[2];
  glGenBuffers(1, &uvo);
  glBindBuffer(GL_ARRAY_BUFFER, uvo);
  glBufferData(GL_ARRAY_BUFFER, np * 8, uv, GL_STATIC_DRAW);
  glGenBuffers(2, vbo);
  glGenTransformFeedbacks(2, fid);
  const GLuint tc = tex2d(cols, rows, GL_RGBA8, GL_RGBA, GL_UNSIGNED_BYTE, img, 1);
  const GLuint td[2] = {tex2d(cols, rows, GL_R32F, GL_RED, GL_FLOAT, dm[0], 1), tex2d(cols, rows, GL_R32F, GL_RED, GL_FLOAT, dm[1], 0)};
  int32_t counts[2] = {0, 0};
  GLuint countQuery;
  glGenQueries(1, &countQuery);

  /* FeedbackBuffer::compute (:84-143), RAW then FILTERED (Context.h:211-223) */
  for (int b = 0; b < 2; b++) {
    void* zero = calloc(np, VERTEX_BYTES);
    glBindBuffer(GL_ARRAY_BUFFER, vbo[b]);
    glBufferData(GL_ARRAY_BUFFER, np * VERTEX_BYTES, zero, GL_STREAM_DRAW);
    free(zero);
    glUseProgram(feedback_prog);
    glUniform4f(glGetUniformLocation(feedback_prog, "cam"), fl[6], fl[7], 1.0f / fl[4], 1.0f / fl[5]);
    glUniform1f(glGetUniformLocation(feedback_prog, "threshold"), 0.0f);
    glUniform1f(glGetUniformLocation(feedback_prog, "cols"), (float)cols);
    glUniform1f(glGetUniformLocation(feedback_prog, "rows"), (float)rows);
    glUniform1i(glGetUniformLocation(feedback_prog, "time"), 1);
    glUniform1i(glGetUniformLocation(feedback_prog, "timeIdx"), 0);
    glUniform1i(glGetUniformLocation(feedback_prog, "gSampler"), 0);
    glUniform1i(glGetUniformLocation(feedback_prog, "cSampler"), 1);
    glUniform1f(glGetUniformLocation(feedback_prog, "maxDepth"), fl[8]);
    glEnableVertexAttribArray(0);
    glBindBuffer(GL_ARRAY_BUFFER, uvo);
    glVertexAttribPointer(0, 2, GL_FLOAT, GL_FALSE, 0, 0);
    p_glEnable(GL_RASTERIZER_DISCARD);
    glBindTransformFeedback(GL_TRANSFORM_FEEDBACK, fid[b]);
    glBindBufferBase(GL_TRANSFORM_FEEDBACK_BUFFER, 0, vbo[b]);
    glBeginTransformFeedback(GL_POINTS);
    glBeginQuery(GL_TRANSFORM_FEEDBACK_PRIMITIVES_WRITTEN, countQuery);
    p_glActiveTexture(GL_TEXTURE0);
    p_glBindTexture(GL_TEXTURE_2D, td[b]);
    p_glActiveTexture(GL_TEXTURE1);
    p_glBindTexture(GL_TEXTURE_2D, tc);
    p_glDrawArrays(GL_POINTS, 0, (GLsizei)np);
    p_glBindTexture(GL_TEXTURE_2D, 0);
    p_glActiveTexture(GL_TEXTURE0);
    glEndQuery(GL_TRANSFORM_FEEDBACK_PRIMITIVES_WRITTEN);
    glEndTransformFeedback();
    p_glDisable(GL_RASTERIZER_DISCARD);
    glDisableVertexAttribArray(0);
    glBindBuffer(GL_ARRAY_BUFFER, 0);
    glBindTransformFeedback(GL_TRANSFORM_FEEDBACK, 0);
    p_glFinish();
    GLuint written = 0;
    glGetQueryObjectuiv(countQuery, GL_QUERY_RESULT, &written);
    counts[b] = (int32_t)written;
  }
  if (p_glGetError() != GL_NO_ERROR) die("GL error in the feedback pass", NULL);

  GLuint fbo, rb[2];
  glGenFramebuffers(1, &fbo);
  glBindFramebuffer(GL_FRAMEBUFFER, fbo);
  glGenRenderbuffers(2, rb);
  glBindRenderbuffer(GL_RENDERBUFFER, rb[0]);
  glRenderbufferStorage(GL_RENDERBUFFER, GL_RGBA8, W, H);
  glFramebufferRenderbuffer(GL_FRAMEBUFFER, GL_COLOR_ATTACHMENT0, GL_RENDERBUFFER, rb[0]);
  glBindRenderbuffer(GL_RENDERBUFFER, rb[1]);
  glRenderbufferStorage(GL_RENDERBUFFER, GL_DEPTH_COMPONENT24, W, H);
  glFramebufferRenderbuffer(GL_FRAMEBUFFER, GL_DEPTH_ATTACHMENT, GL_RENDERBUFFER, rb[1]);
  const GLenum buf0 = GL_COLOR_ATTACHMENT0;
  glDrawBuffers(1, &buf0);
  if (glCheckFramebufferStatus(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) die("framebuffer incomplete", NULL);
  p_glViewport(0, 0, W, H);
  p_glEnable(GL_DEPTH_TEST);
  p_glDepthMask(GL_TRUE);
  p_glDepthFunc(GL_LESS);
  p_glPointSize(1.0f);
  p_glClearColor(fl[0], fl[1], fl[2], fl[3]);
  p_glClear(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT);

  for (int d = 0; d < nd; d++) {
    int32_t ip[2];
    float fp[32];
    rd(ip, sizeof ip, f);
    rd(fp, sizeof fp, f);
    const int b = ip[0] ? 1 : 0;
    /* FeedbackBuffer::render (:145-187): threshold and cluster are never set (0 and false) */
    glUseProgram(draw_prog);
    um4(draw_prog, "MVP", fp);
    um4(draw_prog, "pose", fp + 16);
    glUniform1i(glGetUniformLocation(draw_prog, "colorType"), ip[1]);
    glBindBuffer(GL_ARRAY_BUFFER, vbo[b]);
    glEnableVertexAttribArray(0);
    glVertexAttribPointer(0, 4, GL_FLOAT, GL_FALSE, VERTEX_BYTES, (void*)0);
    glEnableVertexAttribArray(1);
    glVertexAttribPointer(1, 4, GL_FLOAT, GL_FALSE, VERTEX_BYTES, (void*)16);
    for (int i = 0; i < 3; i++) {
      glEnableVertexAttribArray(2 + i);
      glVertexAttribPointer(2 + i, 1, GL_FLOAT, GL_FALSE, VERTEX_BYTES, (void*)(size_t)(32 + 4 * i));
    }
    glEnableVertexAttribArray(5);
    glVertexAttribPointer(5, 4, GL_FLOAT, GL_FALSE, VERTEX_BYTES, (void*)44);
    glDrawTransformFeedback(GL_POINTS, fid[b]);
    for (int i = 0; i < 6; i++) glDisableVertexAttribArray(i);
    glBindBuffer(GL_ARRAY_BUFFER, 0);
  }
  fclose(f);
  p_glFinish();
  if (p_glGetError() != GL_NO_ERROR) die("GL error", NULL);
  uint8_t* rgba = (uint8_t*)malloc((size_t)W * H * 4);
  uint32_t* depth = (uint32_t*)malloc((size_t)W * H * 4);
  p_glPixelStorei(GL_PACK_ALIGNMENT, 1);
  p_glReadBuffer(GL_COLOR_ATTACHMENT0);
  p_glReadPixels(0, 0, W, H, GL_RGBA, GL_UNSIGNED_BYTE, rgba);
  p_glReadPixels(0, 0, W, H, GL_DEPTH_COMPONENT, GL_UNSIGNED_INT, depth);
  if (p_glGetError() != GL_NO_ERROR) die("GL error at read-back", NULL);
  for (size_t i = 0; i < (size_t)W * H; i++) depth[i] >>= 8;
  FILE* o = fopen(argv[3], "wb");
  if (!o) die("cannot write", argv[3]);
  fwrite(rgba, 1, (size_t)W * H * 4, o);
  fwrite(depth, 4, (size_t)W * H, o);
  fwrite(counts, 4, 2, o);
  fclose(o);
  return 0;
}
