/* Test infrastructure: the GL host of tests/golden/make_ref_render_golden.py (which compiles it into a temporary directory).
 *
 * Runs the REFERENCE's own draw programs - draw_global_surface.{vert,geom,frag} and draw_feedback.{vert,frag}, read at RUN time from
 * the shader directory given on the command line (never copied into this repository) - on Mesa's llvmpipe, with the call sequence of
 * GlobalModel::renderPointCloud (GlobalModel.cpp:419-505) and the GUI's framebuffer state: an RGBA8 colour attachment, a
 * DEPTH_COMPONENT24 depth buffer, depth test on, GL_LESS, depth mask on (GUI/src/Tools/GUI.h:73-75), point size 1.  The context is made
 * as oracle/ref_gl_harness.c makes it (Mesa's DRI interface, no X server).  Differences from the reference's host code:
 * glDrawTransformFeedback(GL_POINTS, vbos[target].second) is glDrawArrays(GL_POINTS, 0, count) over a buffer of `count` surfels; the
 * "pose" uniform of the point program is the identity, as renderPointCloud sets it.
 *
 *   gl_render_host SHADER_DIR REQUEST OUTPUT
 * REQUEST (little endian): int32 W, H, n_surfels, n_draws; float32 clear_rgba[4]; n_surfels x 15 float32 (the reference's Vertex:
 * pos.xyz conf | colour 0 initTime stamp | times[3] | normal.xyz radius); per draw: int32 points, colorType, unstable, drawWindow, time,
 * timeIdx, timeDelta, cluster; float32 threshold, cluster_color[3], mvp[16] (row-major).  All draws go into one framebuffer.
 * OUTPUT: W*H RGBA8 (glReadPixels, rows bottom-up) then W*H uint32 24-bit depth (GL_UNSIGNED_INT read shifted right by 8).
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
  X(PFNGLCHECKFRAMEBUFFERSTATUSPROC, glCheckFramebufferStatus) X(PFNGLDRAWBUFFERSPROC, glDrawBuffers)
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

static char g_dir[1024];

static void die(const char* what, const char* detail) {
  fprintf(stderr, "gl_render_host: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
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
/* loadProgramGeomFromFile / loadProgramFromFile (Shaders/Shaders.h) */
static GLuint program(const char* vs, const char* gs, const char* fs) {
  GLuint p = glCreateProgram();
  glAttachShader(p, compile(GL_VERTEX_SHADER, vs));
  if (gs) glAttachShader(p, compile(GL_GEOMETRY_SHADER, gs));
  glAttachShader(p, compile(GL_FRAGMENT_SHADER, fs));
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

int main(int argc, char** argv) {
  if (argc != 4) die("usage: gl_render_host SHADER_DIR REQUEST OUTPUT", NULL);
  snprintf(g_dir, sizeof g_dir, "%s", argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) die("cannot open request", argv[2]);
  int32_t hdr[4];
  float clear[4];
  rd(hdr, sizeof hdr, f);
  rd(clear, sizeof clear, f);
  const int W = hdr[0], H = hdr[1], n = hdr[2], nd = hdr[3];
  float* surf = (float*)malloc((size_t)(n > 0 ? n : 1) * 60);
  rd(surf, (size_t)n * 60, f);

  make_context();
  GLuint vao;
  glGenVertexArrays(1, &vao);
  glBindVertexArray(vao);
  const GLuint surfel_prog = program("draw_global_surface.vert", "draw_global_surface.geom", "draw_global_surface.frag");
  const GLuint point_prog = program("draw_feedback.vert", NULL, "draw_feedback.frag");

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
  p_glClearColor(clear[0], clear[1], clear[2], clear[3]);
  p_glClear(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT);

  GLuint vbo;
  glGenBuffers(1, &vbo);
  glBindBuffer(GL_ARRAY_BUFFER, vbo);
  glBufferData(GL_ARRAY_BUFFER, (size_t)(n > 0 ? n : 1) * 60, surf, GL_STATIC_DRAW);

  for (int d = 0; d < nd; d++) {
    int32_t ip[8];
    float fp[20];
    rd(ip, sizeof ip, f);
    rd(fp, sizeof fp, f);
    /* GlobalModel::renderPointCloud (GlobalModel.cpp:425-503) */
    const GLuint p = ip[0] ? point_prog : surfel_prog;
    glUseProgram(p);
    um4(p, "MVP", fp + 4);
    glUniform1f(glGetUniformLocation(p, "threshold"), fp[0]);
    glUniform1i(glGetUniformLocation(p, "colorType"), ip[1]);
    glUniform1i(glGetUniformLocation(p, "unstable"), ip[2]);
    glUniform1i(glGetUniformLocation(p, "drawWindow"), ip[3]);
    glUniform1i(glGetUniformLocation(p, "time"), ip[4]);
    glUniform1i(glGetUniformLocation(p, "timeIdx"), ip[5]);
    glUniform1i(glGetUniformLocation(p, "timeDelta"), ip[6]);
    const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    um4(p, "pose", ident);
    glUniform1i(glGetUniformLocation(p, "cluster"), ip[7]);
    if (ip[7]) glUniform3f(glGetUniformLocation(p, "cluster_color"), fp[1], fp[2], fp[3]);
    glEnableVertexAttribArray(0);
    glVertexAttribPointer(0, 4, GL_FLOAT, GL_FALSE, 60, (void*)0);
    glEnableVertexAttribArray(1);
    glVertexAttribPointer(1, 4, GL_FLOAT, GL_FALSE, 60, (void*)16);
    for (int i = 0; i < 3; i++) {
      glEnableVertexAttribArray(2 + i);
      glVertexAttribPointer(2 + i, 1, GL_FLOAT, GL_FALSE, 60, (void*)(size_t)(32 + 4 * i));
    }
    glEnableVertexAttribArray(5);
    glVertexAttribPointer(5, 4, GL_FLOAT, GL_FALSE, 60, (void*)44);
    p_glDrawArrays(GL_POINTS, 0, n);
    for (int i = 0; i < 6; i++) glDisableVertexAttribArray(i);
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
  fclose(o);
  return 0;
}
