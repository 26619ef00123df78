/* Test infrastructure: the GL host of tests/golden/make_ref_render_shaded_golden.py (which compiles it into a temporary directory).
 *
 * Runs the REFERENCE's own programs of GUI::drawFXAA (GUI/src/Tools/GUI.h:365-478) - draw_global_surface.{vert,geom} +
 * draw_global_surface_phong.frag and empty.vert + quad.geom + fxaa.frag, read at RUN time from the shader directory given on the
 * command line (never copied into this repository) - on Mesa's llvmpipe with drawFXAA's call sequence and the GUI's state
 * (GUI.h:55-75): an offscreen framebuffer of an RGBA32F texture whose only parameters are the LINEAR min / mag filters (pangolin's
 * GlTexture with sampling_linear; the wrap modes stay GL's default, REPEAT) and a DEPTH_COMPONENT24 renderbuffer; a view framebuffer
 * of RGBA8 + DEPTH_COMPONENT24 standing for the window; depth test on, GL_LESS, depth mask on.  The context and the loading of the
 * shader files (with `#include "x"` expanded by textual insertion, as Pangolin does) are those of tests/golden/gl_render_host.c.
 * Mesa's core profile rejects `texture2D` under `#version 440 core`, so every `texture2D(` of a shader is read as `texture(` (the
 * only other textual edit).  Differences from the reference's host code: glDrawTransformFeedback is glDrawArrays(GL_POINTS, 0, n)
 * over a buffer of n surfels; the view is a framebuffer object, not the window, and the blit's destination is its W x H.
 *
 *   gl_render_shaded_host SHADER_DIR REQUEST OUTPUT
 * REQUEST (little endian): int32 SW, SH (offscreen), W, H (view), n_surfels, colorType, unstable, drawWindow, time, timeIdx,
 * timeDelta; float32 threshold, signMult, lightpos[3], clear[4] (offscreen), view_clear[4], mvp[16] (row-major); n_surfels x 15
 * float32 (the reference's Vertex: pos.xyz conf | colour 0 initTime stamp | times[3] | normal.xyz radius).
 * OUTPUT: SW*SH RGBA32F (glReadPixels GL_FLOAT), SW*SH uint32 24-bit depth, W*H RGBA8, W*H uint32 24-bit depth (rows bottom-up).
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
  X(PFNGLCHECKFRAMEBUFFERSTATUSPROC, glCheckFramebufferStatus) X(PFNGLDRAWBUFFERSPROC, glDrawBuffers)                           \
  X(PFNGLFRAMEBUFFERTEXTURE2DPROC, glFramebufferTexture2D) X(PFNGLBLITFRAMEBUFFERPROC, glBlitFramebuffer)                         \
  X(PFNGLUNIFORM2FPROC, glUniform2f)
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
static void (*p_glActiveTexture)(GLenum);
static void (*p_glGenTextures)(GLsizei, GLuint*);
static void (*p_glBindTexture)(GLenum, GLuint);
static void (*p_glTexImage2D)(GLenum, GLint, GLint, GLsizei, GLsizei, GLint, GLenum, GLenum, const void*);
static void (*p_glTexParameteri)(GLenum, GLenum, GLint);

static char g_dir[1024];

static void die(const char* what, const char* detail) {
  fprintf(stderr, "gl_render_shaded_host: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
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
  LOAD1(glActiveTexture) LOAD1(glGenTextures) LOAD1(glBindTexture) LOAD1(glTexImage2D) LOAD1(glTexParameteri)
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
/* the one textual edit besides #include: `texture2D(` -> `texture(`, which a core profile no longer declares (fxaa.frag:49-81) */
static void core_texture(char* s) {
  for (char* p = strstr(s, "texture2D("); p; p = strstr(p, "texture2D(")) memmove(p + 7, p + 9, strlen(p + 9) + 1);
}
static GLuint compile(GLenum type, const char* name) {
  char* src = expand(name, 0);
  core_texture(src);
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

static void read_depth24(int w, int h, uint32_t* out) {
  p_glReadPixels(0, 0, w, h, GL_DEPTH_COMPONENT, GL_UNSIGNED_INT, out);
  for (size_t i = 0; i < (size_t)w * h; i++) out[i] >>= 8;
}

int main(int argc, char** argv) {
  if (argc != 4) die("usage: gl_render_shaded_host SHADER_DIR REQUEST OUTPUT", NULL);
  snprintf(g_dir, sizeof g_dir, "%s", argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) die("cannot open request", argv[2]);
  int32_t ip[11];
  float fp[29];
  rd(ip, sizeof ip, f);
  rd(fp, sizeof fp, f);
  const int SW = ip[0], SH = ip[1], W = ip[2], H = ip[3], n = ip[4];
  float* surf = (float*)malloc((size_t)(n > 0 ? n : 1) * 60);
  rd(surf, (size_t)n * 60, f);
  fclose(f);

  make_context();
  GLuint vao;
  glGenVertexArrays(1, &vao);
  glBindVertexArray(vao);
  const GLuint colour_prog = program("draw_global_surface.vert", "draw_global_surface.geom", "draw_global_surface_phong.frag");
  const GLuint fxaa_prog = program("empty.vert", "quad.geom", "fxaa.frag");

  /* GUI.h:55-62: the offscreen colour texture and depth buffer */
  GLuint tex, off_fbo, view_fbo, rb[3];
  p_glGenTextures(1, &tex);
  p_glBindTexture(GL_TEXTURE_2D, tex);
  p_glTexImage2D(GL_TEXTURE_2D, 0, GL_RGBA32F, SW, SH, 0, GL_LUMINANCE, GL_FLOAT, NULL);
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MAG_FILTER, GL_LINEAR);
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MIN_FILTER, GL_LINEAR);
  p_glBindTexture(GL_TEXTURE_2D, 0);
  glGenRenderbuffers(3, rb);
  glGenFramebuffers(1, &off_fbo);
  glBindFramebuffer(GL_FRAMEBUFFER, off_fbo);
  glFramebufferTexture2D(GL_FRAMEBUFFER, GL_COLOR_ATTACHMENT0, GL_TEXTURE_2D, tex, 0);
  glBindRenderbuffer(GL_RENDERBUFFER, rb[0]);
  glRenderbufferStorage(GL_RENDERBUFFER, GL_DEPTH_COMPONENT24, SW, SH);
  glFramebufferRenderbuffer(GL_FRAMEBUFFER, GL_DEPTH_ATTACHMENT, GL_RENDERBUFFER, rb[0]);
  const GLenum buf0 = GL_COLOR_ATTACHMENT0;
  glDrawBuffers(1, &buf0);
  if (glCheckFramebufferStatus(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) die("offscreen framebuffer incomplete", NULL);
  /* the view (the window's framebuffer), cleared as the GUI's frame begins */
  glGenFramebuffers(1, &view_fbo);
  glBindFramebuffer(GL_FRAMEBUFFER, view_fbo);
  glBindRenderbuffer(GL_RENDERBUFFER, rb[1]);
  glRenderbufferStorage(GL_RENDERBUFFER, GL_RGBA8, W, H);
  glFramebufferRenderbuffer(GL_FRAMEBUFFER, GL_COLOR_ATTACHMENT0, GL_RENDERBUFFER, rb[1]);
  glBindRenderbuffer(GL_RENDERBUFFER, rb[2]);
  glRenderbufferStorage(GL_RENDERBUFFER, GL_DEPTH_COMPONENT24, W, H);
  glFramebufferRenderbuffer(GL_FRAMEBUFFER, GL_DEPTH_ATTACHMENT, GL_RENDERBUFFER, rb[2]);
  glDrawBuffers(1, &buf0);
  if (glCheckFramebufferStatus(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) die("view framebuffer incomplete", NULL);
  p_glEnable(GL_DEPTH_TEST);
  p_glDepthMask(GL_TRUE);
  p_glDepthFunc(GL_LESS);
  p_glViewport(0, 0, W, H);
  p_glClearColor(fp[9], fp[10], fp[11], fp[12]);
  p_glClear(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT);

  GLuint vbo;
  glGenBuffers(1, &vbo);
  glBindBuffer(GL_ARRAY_BUFFER, vbo);
  glBufferData(GL_ARRAY_BUFFER, (size_t)(n > 0 ? n : 1) * 60, surf, GL_STATIC_DRAW);

  /* GUI::drawFXAA (GUI.h:369-447): first pass into the offscreen buffer */
  glBindFramebuffer(GL_FRAMEBUFFER, off_fbo);
  p_glViewport(0, 0, SW, SH);
  p_glClearColor(fp[5], fp[6], fp[7], fp[8]);
  p_glClear(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT);
  glUseProgram(colour_prog);
  um4(colour_prog, "MVP", fp + 13);
  glUniform1f(glGetUniformLocation(colour_prog, "threshold"), fp[0]);
  glUniform1i(glGetUniformLocation(colour_prog, "time"), ip[8]);
  glUniform1i(glGetUniformLocation(colour_prog, "timeIdx"), ip[9]);
  glUniform1i(glGetUniformLocation(colour_prog, "timeDelta"), ip[10]);
  glUniform1f(glGetUniformLocation(colour_prog, "signMult"), fp[1]);
  glUniform1i(glGetUniformLocation(colour_prog, "colorType"), ip[5]);
  glUniform1i(glGetUniformLocation(colour_prog, "unstable"), ip[6]);
  glUniform1i(glGetUniformLocation(colour_prog, "drawWindow"), ip[7]);
  glUniform3f(glGetUniformLocation(colour_prog, "lightpos"), fp[2], fp[3], fp[4]);
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
  glBindBuffer(GL_ARRAY_BUFFER, 0);

  /* GUI.h:449-473: FXAA into the view, then the depth blit */
  glBindFramebuffer(GL_FRAMEBUFFER, view_fbo);
  p_glViewport(0, 0, W, H);
  glUseProgram(fxaa_prog);
  p_glActiveTexture(GL_TEXTURE0);
  p_glBindTexture(GL_TEXTURE_2D, tex);
  glUniform1i(glGetUniformLocation(fxaa_prog, "tex"), 0);
  glUniform2f(glGetUniformLocation(fxaa_prog, "resolution"), (float)SW, (float)SH);
  p_glDrawArrays(GL_POINTS, 0, 1);
  glBindFramebuffer(GL_READ_FRAMEBUFFER, off_fbo);
  glBindFramebuffer(GL_DRAW_FRAMEBUFFER, view_fbo);
  glBlitFramebuffer(0, 0, SW, SH, 0, 0, W, H, GL_DEPTH_BUFFER_BIT, GL_NEAREST);
  p_glBindTexture(GL_TEXTURE_2D, 0);
  p_glFinish();
  if (p_glGetError() != GL_NO_ERROR) die("GL error", NULL);

  float* off_rgba = (float*)malloc((size_t)SW * SH * 16);
  uint32_t* off_depth = (uint32_t*)malloc((size_t)SW * SH * 4);
  uint8_t* rgba = (uint8_t*)malloc((size_t)W * H * 4);
  uint32_t* depth = (uint32_t*)malloc((size_t)W * H * 4);
  p_glPixelStorei(GL_PACK_ALIGNMENT, 1);
  glBindFramebuffer(GL_FRAMEBUFFER, off_fbo);
  p_glReadBuffer(GL_COLOR_ATTACHMENT0);
  p_glReadPixels(0, 0, SW, SH, GL_RGBA, GL_FLOAT, off_rgba);
  read_depth24(SW, SH, off_depth);
  glBindFramebuffer(GL_FRAMEBUFFER, view_fbo);
  p_glReadBuffer(GL_COLOR_ATTACHMENT0);
  p_glReadPixels(0, 0, W, H, GL_RGBA, GL_UNSIGNED_BYTE, rgba);
  read_depth24(W, H, depth);
  if (p_glGetError() != GL_NO_ERROR) die("GL error at read-back", NULL);
  FILE* o = fopen(argv[3], "wb");
  if (!o) die("cannot write", argv[3]);
  fwrite(off_rgba, 16, (size_t)SW * SH, o);
  fwrite(off_depth, 4, (size_t)SW * SH, o);
  fwrite(rgba, 4, (size_t)W * H, o);
  fwrite(depth, 4, (size_t)W * H, o);
  fclose(o);
  return 0;
}
