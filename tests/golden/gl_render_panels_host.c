/* Test infrastructure: the GL host of tests/golden/make_ref_render_panels_golden.py (which compiles it into a temporary directory).
 *
 * Runs the REFERENCE's own panel programs - empty.vert + quad.geom with depth_norm.frag and with visualise_textures.frag, read at RUN
 * time from the shader directory given on the command line (never copied into this repository) - on Mesa's llvmpipe, with the call
 * sequences of ComputePack::compute (Core/src/Shaders/ComputePack.cpp:41-73) and IndexMap::renderDepth (Core/src/IndexMap.cpp:219-251),
 * then draws a texture into a window-sized RGBA8 framebuffer through a flipped textured quad in GUI::displayImg's state (depth test
 * off, GUI/src/Tools/GUI.h:340-350).  The context is a 4.5 COMPATIBILITY context where the driver gives one: the quad is then drawn
 * by the fixed-function pipeline (GL_MODULATE with the current colour), DEPTH_NORM is the reference's unsized GL_LUMINANCE texture and
 * flags[0] = 1.  Otherwise (or with PANELS_HOST_CORE=1 in the environment) the context is 4.5 core as in tests/golden/gl_render_host.c,
 * the quad is drawn by the pass-through program below (texture times colour) and luminance is an R8 texture swizzled to (R, R, R, 1).
 * flags[1] = 1 when the framebuffer with the GL_LUMINANCE attachment was complete and depth_norm.frag rendered into it; otherwise the
 * shader's float output is captured in an R32F attachment and converted to bytes here by floor(clamp(v, 0, 1) * 255 + 0.5).
 * Textures: MIN / MAG filter per request, CLAMP_TO_EDGE.  The shader text is compiled as read, with one line added after `#version`
 * (see compile()).
 *
 *   gl_render_panels_host SHADER_DIR REQUEST OUTPUT
 * REQUEST (little endian): int32 cols, rows, n_blits; float32 minVal, maxVal (normaliseDepth's uniforms, already scaled), maxDepth;
 * cols*rows uint16 raw depth; cols*rows*4 float32 vertex image; cols*rows RGBA8 colour; cols*rows RGBA8 predicted colour (image
 * rows, top first); per blit: int32 source (0 DEPTH_NORM, 1 Model, 2 colour, 3 predicted colour), linear, W, H, vx, vy, vw, vh;
 * float32 colour[3], clear[4].
 * OUTPUT: int32 flags[4]; cols*rows bytes DEPTH_NORM; cols*rows RGBA8 Model image (both as texture rows = image rows); per blit W*H
 * RGBA8 (glReadPixels, rows bottom-up).
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
  X(PFNGLGETQUERYOBJECTUIVPROC, glGetQueryObjectuiv) X(PFNGLFRAMEBUFFERTEXTURE2DPROC, glFramebufferTexture2D)
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
static void (*p_glGetTexImage)(GLenum, GLint, GLenum, GLenum, void*);
/* compatibility profile only */
static void (*p_glMatrixMode)(GLenum);
static void (*p_glLoadIdentity)(void);
static void (*p_glColor3f)(GLfloat, GLfloat, GLfloat);
static void (*p_glEnableClientState)(GLenum);
static void (*p_glDisableClientState)(GLenum);
static void (*p_glVertexPointer)(GLint, GLenum, GLsizei, const void*);
static void (*p_glTexCoordPointer)(GLint, GLenum, GLsizei, const void*);
static int g_compat;

static char g_dir[1024];

static void die(const char* what, const char* detail) {
  fprintf(stderr, "gl_render_panels_host: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
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
  __DRIcontext* ctx = NULL;
  if (!getenv("PANELS_HOST_CORE")) ctx = sw->createContextAttribs(scr, __DRI_API_OPENGL, configs[0], NULL, 2, attribs, &err, NULL);
  g_compat = ctx != NULL;
  if (!ctx) ctx = sw->createContextAttribs(scr, __DRI_API_OPENGL_CORE, configs[0], NULL, 2, attribs, &err, NULL);
  if (!ctx) die("no OpenGL 4.5 context from llvmpipe", NULL);
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
  LOAD1(glGetTexImage)
  if (g_compat) {
    LOAD1(glMatrixMode) LOAD1(glLoadIdentity) LOAD1(glColor3f) LOAD1(glEnableClientState) LOAD1(glDisableClientState) LOAD1(glVertexPointer)
    LOAD1(glTexCoordPointer)
  }
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
  /* visualise_textures.frag calls texture2D under `#version 440 core`, which Mesa's GLSL does not declare there (the reference's
   * vendor driver does): the overloaded name is mapped to texture() by one line after the #version line, at run time */
  static const char* fix = "#define texture2D texture\n";
  const char* ver = strstr(src, "#version");
  const char* eol = ver ? strchr(ver, '\n') : NULL;
  const char* parts[3] = {src, "", ""};
  GLint lens[3] = {(GLint)strlen(src), 0, 0};
  if (eol) {
    lens[0] = (GLint)(eol + 1 - src);
    parts[1] = fix, lens[1] = (GLint)strlen(fix);
    parts[2] = eol + 1, lens[2] = (GLint)strlen(eol + 1);
  }
  glShaderSource(s, 3, parts, lens);
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
static GLuint link_program(GLuint p, const char* what) {
  glLinkProgram(p);
  GLint ok = 0;
  glGetProgramiv(p, GL_LINK_STATUS, &ok);
  if (!ok) {
    char log[3000];
    glGetProgramInfoLog(p, sizeof log, NULL, log);
    die(what, log);
  }
  return p;
}
/* loadProgramFromFile(vertex, fragment, geometry) (Shaders/Shaders.h) */
static GLuint program(const char* vs, const char* gs, const char* fs) {
  GLuint p = glCreateProgram();
  glAttachShader(p, compile(GL_VERTEX_SHADER, vs));
  if (gs) glAttachShader(p, compile(GL_GEOMETRY_SHADER, gs));
  if (fs) glAttachShader(p, compile(GL_FRAGMENT_SHADER, fs));
  return link_program(p, fs);
}

/* the pass-through program of the core-profile path: texture times colour (this repository's own, not the reference's) */
static GLuint own_program(void) {
  static const char* vs = "#version 330 core\nlayout(location = 0) in vec2 p;\nlayout(location = 1) in vec2 t;\nout vec2 tc;\n"
                          "void main() { gl_Position = vec4(p, 0.0, 1.0); tc = t; }\n";
  static const char* fs = "#version 330 core\nuniform sampler2D s;\nuniform vec4 col;\nin vec2 tc;\nout vec4 o;\n"
                          "void main() { o = texture(s, tc) * col; }\n";
  GLuint p = glCreateProgram();
  const char* srcs[2] = {vs, fs};
  const GLenum types[2] = {GL_VERTEX_SHADER, GL_FRAGMENT_SHADER};
  for (int k = 0; k < 2; k++) {
    GLuint s = glCreateShader(types[k]);
    glShaderSource(s, 1, &srcs[k], NULL);
    glCompileShader(s);
    GLint ok = 0;
    glGetShaderiv(s, GL_COMPILE_STATUS, &ok);
    if (!ok) die("pass-through shader", NULL);
    glAttachShader(p, s);
  }
  return link_program(p, "pass-through program");
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
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MIN_FILTER, linear ? GL_LINEAR : GL_NEAREST);
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MAG_FILTER, linear ? GL_LINEAR : GL_NEAREST);
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_WRAP_S, GL_CLAMP_TO_EDGE);
  p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_WRAP_T, GL_CLAMP_TO_EDGE);
  return t;
}

/* a framebuffer of one colour texture and a depth renderbuffer (ComputePack's, IndexMap's drawFrameBuffer); 0 when incomplete */
static GLuint fbo_of(GLuint tex, int w, int h) {
  GLuint fbo, rb;
  glGenFramebuffers(1, &fbo);
  glBindFramebuffer(GL_FRAMEBUFFER, fbo);
  glFramebufferTexture2D(GL_FRAMEBUFFER, GL_COLOR_ATTACHMENT0, GL_TEXTURE_2D, tex, 0);
  glGenRenderbuffers(1, &rb);
  glBindRenderbuffer(GL_RENDERBUFFER, rb);
  glRenderbufferStorage(GL_RENDERBUFFER, GL_DEPTH_COMPONENT24, w, h);
  glFramebufferRenderbuffer(GL_FRAMEBUFFER, GL_DEPTH_ATTACHMENT, GL_RENDERBUFFER, rb);
  const GLenum buf0 = GL_COLOR_ATTACHMENT0;
  glDrawBuffers(1, &buf0);
  if (glCheckFramebufferStatus(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) {
    glBindFramebuffer(GL_FRAMEBUFFER, 0);
    while (p_glGetError() != GL_NO_ERROR) {
    }
    return 0;
  }
  return fbo;
}

/* ComputePack::compute / IndexMap::renderDepth: viewport, clear to zero, the program, one point */
static void quad_pass(GLuint fbo, int w, int h, GLuint prog) {
  glBindFramebuffer(GL_FRAMEBUFFER, fbo);
  p_glViewport(0, 0, w, h);
  p_glClearColor(0, 0, 0, 0);
  p_glClear(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT);
  glUseProgram(prog);
  p_glDrawArrays(GL_POINTS, 0, 1);
  glBindFramebuffer(GL_FRAMEBUFFER, 0);
  glUseProgram(0);
  p_glFinish();
}

int main(int argc, char** argv) {
  if (argc != 4) die("usage: gl_render_panels_host SHADER_DIR REQUEST OUTPUT", NULL);
  snprintf(g_dir, sizeof g_dir, "%s", argv[1]);
  FILE* f = fopen(argv[2], "rb");
  if (!f) die("cannot open request", argv[2]);
  int32_t hdr[3];
  float fl[3];
  rd(hdr, sizeof hdr, f);
  rd(fl, sizeof fl, f);
  const int cols = hdr[0], rows = hdr[1], nb = hdr[2];
  const size_t np = (size_t)cols * rows;
  uint16_t* depth = (uint16_t*)malloc(np * 2);
  float* vertex = (float*)malloc(np * 16);
  uint8_t* img = (uint8_t*)malloc(np * 4);
  uint8_t* pimg = (uint8_t*)malloc(np * 4);
  rd(depth, np * 2, f);
  rd(vertex, np * 16, f);
  rd(img, np * 4, f);
  rd(pimg, np * 4, f);

  make_context();
  GLuint vao;
  glGenVertexArrays(1, &vao);
  glBindVertexArray(vao);
  int32_t flags[4] = {g_compat, 0, 0, 0};
  const GLuint norm_prog = program("empty.vert", "quad.geom", "depth_norm.frag");
  const GLuint model_prog = program("empty.vert", "quad.geom", "visualise_textures.frag");

  /* normaliseDepth (ElasticFusion.cpp:770-779): DEPTH_RAW is GL_LUMINANCE16UI_EXT, NEAREST (Context.h:162-164); R16UI in core GL */
  const GLuint t_raw = tex2d(cols, rows, GL_R16UI, GL_RED_INTEGER, GL_UNSIGNED_SHORT, depth, 0);
  GLuint t_norm = 0, fbo_norm = 0;
  if (g_compat) { /* Context.h:179-181: GL_LUMINANCE, GL_LUMINANCE, GL_FLOAT, LINEAR */
    t_norm = tex2d(cols, rows, GL_LUMINANCE, GL_LUMINANCE, GL_FLOAT, NULL, 1);
    if (p_glGetError() == GL_NO_ERROR) fbo_norm = fbo_of(t_norm, cols, rows);
  }
  uint8_t* norm = (uint8_t*)malloc(np);
  p_glActiveTexture(GL_TEXTURE0);
  glUseProgram(norm_prog);
  glUniform1f(glGetUniformLocation(norm_prog, "maxVal"), fl[1]);
  glUniform1f(glGetUniformLocation(norm_prog, "minVal"), fl[0]);
  if (fbo_norm) {
    flags[1] = 1;
    p_glBindTexture(GL_TEXTURE_2D, t_raw);
    quad_pass(fbo_norm, cols, rows, norm_prog);
    p_glBindTexture(GL_TEXTURE_2D, t_norm);
    p_glPixelStorei(GL_PACK_ALIGNMENT, 1);
    p_glGetTexImage(GL_TEXTURE_2D, 0, GL_RED, GL_UNSIGNED_BYTE, norm); /* (GL_LUMINANCE would sum the channels on the way out) */
  } else {
    const GLuint t_f = tex2d(cols, rows, GL_R32F, GL_RED, GL_FLOAT, NULL, 0);
    const GLuint fbo = fbo_of(t_f, cols, rows);
    if (!fbo) die("R32F framebuffer incomplete", NULL);
    p_glBindTexture(GL_TEXTURE_2D, t_raw);
    quad_pass(fbo, cols, rows, norm_prog);
    float* nf = (float*)malloc(np * 4);
    p_glBindTexture(GL_TEXTURE_2D, t_f);
    p_glGetTexImage(GL_TEXTURE_2D, 0, GL_RED, GL_FLOAT, nf);
    for (size_t i = 0; i < np; i++) {
      const float c = nf[i] < 0.f ? 0.f : nf[i] > 1.f ? 1.f : nf[i];
      norm[i] = nf[i] == nf[i] ? (uint8_t)(int)(c * 255.f + 0.5f) : 0;
    }
    free(nf);
    if (g_compat) {
      p_glBindTexture(GL_TEXTURE_2D, t_norm);
      p_glTexImage2D(GL_TEXTURE_2D, 0, GL_LUMINANCE, cols, rows, 0, GL_LUMINANCE, GL_UNSIGNED_BYTE, norm);
    } else {
      t_norm = tex2d(cols, rows, GL_R8, GL_RED, GL_UNSIGNED_BYTE, norm, 1);
      p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_SWIZZLE_G, GL_RED);
      p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_SWIZZLE_B, GL_RED);
      p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_SWIZZLE_A, GL_ONE);
    }
  }
  if (p_glGetError() != GL_NO_ERROR) die("GL error in the depth_norm pass", NULL);

  /* renderDepth (IndexMap.cpp:219-251): vertexTexture RGBA32F NEAREST, drawTexture GL_RGBA NEAREST */
  const GLuint t_vert = tex2d(cols, rows, GL_RGBA32F, GL_RGBA, GL_FLOAT, vertex, 0);
  const GLuint t_draw = tex2d(cols, rows, GL_RGBA, GL_RGBA, GL_UNSIGNED_BYTE, NULL, 0);
  const GLuint fbo_draw = fbo_of(t_draw, cols, rows);
  if (!fbo_draw) die("drawTexture framebuffer incomplete", NULL);
  glUseProgram(model_prog);
  glUniform1f(glGetUniformLocation(model_prog, "maxDepth"), fl[2]);
  glUniform1i(glGetUniformLocation(model_prog, "texVerts"), 0);
  p_glBindTexture(GL_TEXTURE_2D, t_vert);
  quad_pass(fbo_draw, cols, rows, model_prog);
  uint8_t* model = (uint8_t*)malloc(np * 4);
  p_glBindTexture(GL_TEXTURE_2D, t_draw);
  p_glGetTexImage(GL_TEXTURE_2D, 0, GL_RGBA, GL_UNSIGNED_BYTE, model);
  if (p_glGetError() != GL_NO_ERROR) die("GL error in the renderDepth pass", NULL);

  /* Context.h:158-160 (RGB: LINEAR), IndexMap.cpp:59-65 (imageTexture: NEAREST); the filter of each blit is the request's */
  const GLuint t_src[4] = {t_norm, t_draw, tex2d(cols, rows, GL_RGBA, GL_RGBA, GL_UNSIGNED_BYTE, img, 1),
                           tex2d(cols, rows, GL_RGBA, GL_RGBA, GL_UNSIGNED_BYTE, pimg, 0)};
  const GLuint own = g_compat ? 0 : own_program();
  GLuint qbuf = 0;
  /* the flipped quad: vertex (x, y) with texcoord (s, t): the bottom of the viewport shows t = 1 */
  static const GLfloat sq_vert[] = {-1, -1, 1, -1, 1, 1, -1, 1}, sq_tex[] = {0, 1, 1, 1, 1, 0, 0, 0};
  if (!g_compat) {
    GLfloat both[16];
    memcpy(both, sq_vert, sizeof sq_vert);
    memcpy(both + 8, sq_tex, sizeof sq_tex);
    glGenBuffers(1, &qbuf);
    glBindBuffer(GL_ARRAY_BUFFER, qbuf);
    glBufferData(GL_ARRAY_BUFFER, sizeof both, both, GL_STATIC_DRAW);
  }

  FILE* o = fopen(argv[3], "wb");
  if (!o) die("cannot write", argv[3]);
  fwrite(flags, 4, 4, o);
  fwrite(norm, 1, np, o);
  fwrite(model, 1, np * 4, o);
  for (int b = 0; b < nb; b++) {
    int32_t ip[8];
    float fp[7];
    rd(ip, sizeof ip, f);
    rd(fp, sizeof fp, f);
    const int W = ip[2], H = ip[3];
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
    if (glCheckFramebufferStatus(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) die("framebuffer incomplete", NULL);
    p_glViewport(0, 0, W, H);
    p_glClearColor(fp[3], fp[4], fp[5], fp[6]);
    p_glClear(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT);
    /* displayImg: glDisable(GL_DEPTH_TEST); Display(id).Activate() sets the viewport; RenderToViewport(true) */
    p_glDisable(GL_DEPTH_TEST);
    p_glViewport(ip[4], ip[5], ip[6], ip[7]);
    p_glActiveTexture(GL_TEXTURE0);
    p_glBindTexture(GL_TEXTURE_2D, t_src[ip[0] & 3]);
    p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MIN_FILTER, ip[1] ? GL_LINEAR : GL_NEAREST);
    p_glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MAG_FILTER, ip[1] ? GL_LINEAR : GL_NEAREST);
    if (g_compat) {
      glBindVertexArray(0);
      glBindBuffer(GL_ARRAY_BUFFER, 0);
      p_glMatrixMode(GL_PROJECTION);
      p_glLoadIdentity();
      p_glMatrixMode(GL_MODELVIEW);
      p_glLoadIdentity();
      p_glColor3f(fp[0], fp[1], fp[2]);
      p_glEnable(GL_TEXTURE_2D);
      p_glTexCoordPointer(2, GL_FLOAT, 0, sq_tex);
      p_glEnableClientState(GL_TEXTURE_COORD_ARRAY);
      p_glVertexPointer(2, GL_FLOAT, 0, sq_vert);
      p_glEnableClientState(GL_VERTEX_ARRAY);
      p_glDrawArrays(GL_TRIANGLE_FAN, 0, 4);
      p_glDisableClientState(GL_VERTEX_ARRAY);
      p_glDisableClientState(GL_TEXTURE_COORD_ARRAY);
      p_glDisable(GL_TEXTURE_2D);
      glBindVertexArray(vao);
    } else {
      glUseProgram(own);
      glUniform1i(glGetUniformLocation(own, "s"), 0);
      glUniform4f(glGetUniformLocation(own, "col"), fp[0], fp[1], fp[2], 1.0f);
      glBindBuffer(GL_ARRAY_BUFFER, qbuf);
      glEnableVertexAttribArray(0);
      glVertexAttribPointer(0, 2, GL_FLOAT, GL_FALSE, 0, (void*)0);
      glEnableVertexAttribArray(1);
      glVertexAttribPointer(1, 2, GL_FLOAT, GL_FALSE, 0, (void*)(8 * sizeof(GLfloat)));
      p_glDrawArrays(GL_TRIANGLE_FAN, 0, 4);
      glDisableVertexAttribArray(0);
      glDisableVertexAttribArray(1);
      glUseProgram(0);
    }
    p_glEnable(GL_DEPTH_TEST);
    p_glFinish();
    if (p_glGetError() != GL_NO_ERROR) die("GL error in a blit", NULL);
    uint8_t* rgba = (uint8_t*)malloc((size_t)W * H * 4);
    p_glPixelStorei(GL_PACK_ALIGNMENT, 1);
    p_glReadBuffer(GL_COLOR_ATTACHMENT0);
    p_glReadPixels(0, 0, W, H, GL_RGBA, GL_UNSIGNED_BYTE, rgba);
    if (p_glGetError() != GL_NO_ERROR) die("GL error at read-back", NULL);
    fwrite(rgba, 1, (size_t)W * H * 4, o);
    free(rgba);
  }
  fclose(f);
  fclose(o);
  return 0;
}
