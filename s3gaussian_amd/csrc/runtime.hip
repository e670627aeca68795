// Runtime of libs3g.so that belongs to no kernel family: the last-error string, the ABI version and the optional in-library
// kernel timing.  Declared in common.hpp; no kernels here.
#include "common.hpp"

#include <stdarg.h>

#include <vector>

namespace s3g {

static thread_local char g_err[512] = {0};
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
void clear_error() { g_err[0] = 0; }

// ---- in-library kernel timing -----------------------------------------------------------------------------
struct ProfRec { hipEvent_t a, b; double instances, pixels; };
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof[S3G_PROFILE_IDS];
static hipEvent_t g_prof_pending[S3G_PROFILE_IDS];
void profile_begin(int id, hipStream_t stream) {
  if (!g_prof_on || id < 0 || id >= S3G_PROFILE_IDS) return;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, stream);
  g_prof_pending[id] = e;
}
void profile_end(int id, hipStream_t stream, double instances, double pixels) {
  if (!g_prof_on || id < 0 || id >= S3G_PROFILE_IDS) return;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return;
  (void)hipEventRecord(e, stream);
  g_prof[id].push_back(ProfRec{g_prof_pending[id], e, instances, pixels});
}

}  // namespace s3g

using namespace s3g;

extern "C" const char* s3g_last_error(void) { return g_err; }
extern "C" int s3g_abi_version(void) { return 16; }

extern "C" void s3g_profile_enable(int on) { g_prof_on = on != 0; }

// Sums the recorded launches of kernel `id` (S3G_PROFILE_* in s3g_raster.h), synchronising on their events, then forgets
// them.  Returns the number of launches.
extern "C" int s3g_profile_read(int id, double* total_ms, double* total_instances, double* total_pixels) {
  if (id < 0 || id >= S3G_PROFILE_IDS) return 0;
  double ms = 0, inst = 0, pix = 0;
  int n = 0;
  for (ProfRec& r : g_prof[id]) {
    float t = 0.f;
    if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) {
      ms += t; inst += r.instances; pix += r.pixels; n++;
    }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  g_prof[id].clear();
  if (total_ms) *total_ms = ms;
  if (total_instances) *total_instances = inst;
  if (total_pixels) *total_pixels = pix;
  return n;
}
