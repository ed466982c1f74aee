/*
 * ref_7z_check.c -- TEST INFRASTRUCTURE ONLY.
 *
 * A stand-alone program around ref_shim.c's two 7z calls (ref_7z_extract,
 * ref_7z_info), built by oracle/Makefile.ref with the host sanitizers
 * (-fsanitize=address,undefined, no recovery) into oracle/_ref/ref_7z_check.
 * tests/golden/make_golden_szh.py runs it once per hand-made archive: a run
 * that a sanitizer ends shows that the reference's answer for that input rests
 * on undefined behaviour, and the golden file is not written.  The answers are
 * printed as one JSON line so that the generator can compare them with what
 * the unsanitized library gave, the largest allocation the reference asked for
 * among them.
 *
 *   ref_7z_check ARCHIVE
 *
 * Leaks are not reported: the reference overwrites its own pointers where a
 * header repeats a section (a second kName, kPackInfo, ...), which loses
 * memory and is no undefined behaviour.  An allocation too large for the
 * sanitizer's allocator returns null, as malloc does, and the reference
 * answers SZ_ERROR_MEM.
 */
#include <stdio.h>
#include <stdlib.h>

int ref_7z_extract(const unsigned char *arc, size_t size, unsigned char *out, size_t cap,
                   size_t *out_len, int *file_res, unsigned long long *file_size,
                   unsigned *n_files, unsigned max_files, unsigned char *names,
                   size_t names_cap, size_t *names_len);
int ref_7z_info(const unsigned char *arc, size_t size, unsigned long long *folders,
                size_t folder_cap, unsigned *n_folders, unsigned *files, size_t file_cap,
                unsigned *n_files);

unsigned long long ref_shim_max_alloc(int reset);

const char *__asan_default_options(void) { return "detect_leaks=0:allocator_may_return_null=1"; }

#define MAX_FILES 512
#define MAX_FOLDERS 256
#define OUT_CAP (1 << 16)
#define NAMES_CAP (1 << 14)

static void hex(const unsigned char *p, size_t n) {
  size_t i;
  putchar('"');
  for (i = 0; i < n; i++) printf("%02x", p[i]);
  putchar('"');
}

int main(int argc, char **argv) {
  static unsigned char out[OUT_CAP], names[NAMES_CAP];
  static int file_res[MAX_FILES];
  static unsigned long long file_size[MAX_FILES], folders[5 * MAX_FOLDERS];
  static unsigned files[5 * MAX_FILES];
  unsigned char *arc;
  size_t size, out_len = 0, names_len = 0;
  unsigned n_files = 0, n_folders = 0, n_files2 = 0, i;
  long len;
  int res, res2;
  FILE *f;
  if (argc != 2 || (f = fopen(argv[1], "rb")) == NULL) return 2;
  fseek(f, 0, SEEK_END);
  len = ftell(f);
  fseek(f, 0, SEEK_SET);
  /* an exact-size heap copy: a read past the archive's end is a finding */
  arc = (unsigned char *)malloc(len > 0 ? (size_t)len : 1);
  size = fread(arc, 1, (size_t)len, f);
  fclose(f);
  ref_shim_max_alloc(1);
  res = ref_7z_extract(arc, size, out, OUT_CAP, &out_len, file_res, file_size, &n_files, MAX_FILES,
                       names, NAMES_CAP, &names_len);
  res2 = ref_7z_info(arc, size, folders, MAX_FOLDERS, &n_folders, files, MAX_FILES, &n_files2);
  if (res != res2 || n_files != n_files2 || n_files > MAX_FILES || n_folders > MAX_FOLDERS) return 3;
  printf("{\"open\": %d, \"folders\": [", res);
  for (i = 0; i < n_folders; i++)
    printf("%s[%llu, %llu, %llu, %llu, %llu]", i ? ", " : "", folders[5 * i], folders[5 * i + 1],
           folders[5 * i + 2], folders[5 * i + 3], folders[5 * i + 4]);
  printf("], \"files\": [");
  for (i = 0; i < n_files; i++)
    printf("%s[%u, %u, %u, %u, %u, %llu, %d]", i ? ", " : "", files[5 * i], files[5 * i + 1],
           files[5 * i + 2], files[5 * i + 3], files[5 * i + 4], file_size[i], file_res[i]);
  printf("], \"names\": ");
  hex(names, names_len);
  printf(", \"out\": ");
  hex(out, out_len);
  printf(", \"max_alloc\": %llu", ref_shim_max_alloc(0));
  printf("}\n");
  free(arc);
  return 0;
}
