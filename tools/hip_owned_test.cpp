/* Host check of csrc/hip_owned.h, built with ASan + UBSan (make
 * hip_owned_test).  Runs anywhere: with no HIP device every creating call
 * fails, and failed creation followed by moves is the path that must not
 * double-free; with a device the same moves run over live handles. */
#include "../go-spacemesh_amd/csrc/hip_owned.h"

#include <cstdio>
#include <utility>

using namespace hip_owned;

static int failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                              \
    }                                                                          \
  } while (0)

/* creation succeeded <=> the owner holds something */
#define CHECK_MADE(err, owner) CHECK(((err) == hipSuccess) == ((owner).get() != nullptr))

template <typename O, typename Make> static void exercise(Make make) {
  { O empty; } /* destruction of an empty handle */

  O a;
  CHECK_MADE(make(a), a); /* without a device: creation failed */
  const auto held = a.get();

  O b(std::move(a)); /* move construction */
  CHECK(a.get() == nullptr && b.get() == held);

  O c;
  CHECK_MADE(make(c), c);
  c = std::move(b); /* move assignment over a live (or failed) handle */
  CHECK(b.get() == nullptr && c.get() == held);

  O &self = c;
  c = std::move(self); /* self-move keeps the handle */
  CHECK(c.get() == held);

  CHECK_MADE(make(c), c); /* creating again releases what was held */
  O d;
  d = std::move(a); /* assignment from a moved-from handle */
  CHECK(d.get() == nullptr);

  O e;
  CHECK_MADE(make(e), e);
  e.reset();
  e.reset(); /* twice is once */
  CHECK(e.get() == nullptr);
  CHECK(e.release() == nullptr);
} /* c, perhaps live, and the empty ones are destroyed here */

int main() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess) devices = 0;
  exercise<DevBuf<int>>([](DevBuf<int> &o) { return o.alloc(4096); });
  exercise<PinnedBuf<int>>([](PinnedBuf<int> &o) { return o.alloc(4096); });
  exercise<Event>([](Event &o) { return o.create(hipEventDisableTiming); });
  exercise<Stream>([](Stream &o) { return o.create(); });
  std::printf("hip_owned_test: %d device(s), %d failure(s)\n", devices,
              failures);
  return failures ? 1 : 0;
}
