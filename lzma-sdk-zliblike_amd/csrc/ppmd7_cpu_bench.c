/* ppmd7_cpu_bench.c -- CPU baseline of ppmd7_bench.py: the reference's PPMd7
 * decoder as built into oracle/_ref/libref.so, one stream after another per
 * thread.  The exported functions are looked up at run time and CPpmd7 is an
 * opaque block, so no reference header is needed; the range decoder's layout
 * (three function pointers, Range, Code, the byte stream) is stated here.
 *
 *   ppmd7_cpu_bench LIBREF PACKED ORDER MEM PLAIN_LEN COPIES THREADS REPS OUT
 *
 * decodes COPIES copies of the stream in PACKED on THREADS threads, REPS times;
 * prints the best wall time in seconds; writes copy 0's output to OUT and
 * fails unless every copy decoded cleanly to the same bytes. */
#include <dlfcn.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

typedef struct { unsigned char (*Read)(void *p); } ByteIn;
typedef struct { void *(*Alloc)(void *p, size_t n); void (*Free)(void *p, void *a); } Alloc;
typedef struct {
  void *get_threshold, *decode, *decode_bit;
  uint32_t range, code;
  ByteIn *stream;
} RangeDec;
typedef struct { ByteIn in; const unsigned char *cur, *end; int extra; } MemIn;

static unsigned char mem_read(void *pp) {
  MemIn *s = (MemIn *)pp;
  if (s->cur != s->end) return *s->cur++;
  s->extra = 1;
  return 0;
}
static void *a_alloc(void *p, size_t n) { (void)p; return malloc(n); }
static void a_free(void *p, void *a) { (void)p; free(a); }

static void (*f_construct)(void *);
static int (*f_alloc)(void *, uint32_t, Alloc *);
static void (*f_free)(void *, Alloc *);
static void (*f_init)(void *, unsigned);
static void (*f_vtable)(RangeDec *);
static int (*f_rc_init)(RangeDec *);
static int (*f_symbol)(void *, RangeDec *);

static const unsigned char *g_src;
static size_t g_src_len, g_plain_len;
static unsigned g_order, g_copies, g_threads;
static uint32_t g_mem;
static unsigned char *g_out;
static int g_bad;

static void *worker(void *arg) {
  const unsigned t = (unsigned)(size_t)arg;
  Alloc al = { a_alloc, a_free };
  void *model = calloc(1, 64 << 10);  /* CPpmd7 is about 19 KiB */
  unsigned k;
  f_construct(model);
  if (!f_alloc(model, g_mem, &al)) { g_bad = 1; return 0; }
  for (k = t; k < g_copies; k += g_threads) {
    unsigned char *out = g_out + (size_t)k * g_plain_len;
    RangeDec rc;
    MemIn s;
    size_t i = 0;
    s.in.Read = mem_read; s.cur = g_src; s.end = g_src + g_src_len; s.extra = 0;
    f_init(model, g_order);
    f_vtable(&rc);
    rc.stream = &s.in;
    if (f_rc_init(&rc) && !s.extra)
      for (; i < g_plain_len; i++) {
        const int sym = f_symbol(model, &rc);
        if (s.extra || sym < 0) break;
        out[i] = (unsigned char)sym;
      }
    if (i != g_plain_len || s.cur != s.end || rc.code != 0) g_bad = 1;
  }
  f_free(model, &al);
  free(model);
  return 0;
}

int main(int argc, char **argv) {
  void *h;
  FILE *f;
  unsigned reps, r, t;
  double best = 1e30;
  unsigned char *src;
  if (argc < 10) return 2;
  h = dlopen(argv[1], RTLD_LAZY);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 3; }
  *(void **)&f_construct = dlsym(h, "Ppmd7_Construct");
  *(void **)&f_alloc = dlsym(h, "Ppmd7_Alloc");
  *(void **)&f_free = dlsym(h, "Ppmd7_Free");
  *(void **)&f_init = dlsym(h, "Ppmd7_Init");
  *(void **)&f_vtable = dlsym(h, "Ppmd7z_RangeDec_CreateVTable");
  *(void **)&f_rc_init = dlsym(h, "Ppmd7z_RangeDec_Init");
  *(void **)&f_symbol = dlsym(h, "Ppmd7_DecodeSymbol");
  if (!f_construct || !f_alloc || !f_free || !f_init || !f_vtable || !f_rc_init || !f_symbol) return 3;
  f = fopen(argv[2], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END); g_src_len = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
  src = (unsigned char *)malloc(g_src_len + 1);
  if (fread(src, 1, g_src_len, f) != g_src_len) return 3;
  fclose(f);
  g_src = src;
  g_order = (unsigned)atoi(argv[3]);
  g_mem = (uint32_t)strtoul(argv[4], 0, 10);
  g_plain_len = (size_t)strtoull(argv[5], 0, 10);
  g_copies = (unsigned)atoi(argv[6]);
  g_threads = (unsigned)atoi(argv[7]);
  reps = (unsigned)atoi(argv[8]);
  if (g_threads < 1 || g_threads > 256 || g_copies < 1) return 2;
  g_out = (unsigned char *)malloc((size_t)g_copies * g_plain_len + 1);
  for (r = 0; r < reps; r++) {
    pthread_t th[256];
    struct timespec a, b;
    double dt;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (t = 0; t < g_threads; t++) pthread_create(&th[t], 0, worker, (void *)(size_t)t);
    for (t = 0; t < g_threads; t++) pthread_join(th[t], 0);
    clock_gettime(CLOCK_MONOTONIC, &b);
    dt = (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec);
    if (dt < best) best = dt;
  }
  for (t = 1; t < g_copies; t++)
    if (memcmp(g_out, g_out + (size_t)t * g_plain_len, g_plain_len) != 0) g_bad = 1;
  f = fopen(argv[9], "wb");
  if (!f) return 3;
  fwrite(g_out, 1, g_plain_len, f);
  fclose(f);
  if (g_bad) { fprintf(stderr, "decode mismatch\n"); return 1; }
  printf("%.6f\n", best);
  return 0;
}
