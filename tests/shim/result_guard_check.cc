// result_guard_check.cc — a stand-alone program for tests/test_host_surface_cpu.py (built with
// -fsanitize=address,undefined and run): the scope guard of csrc/host/result_guard.h around a result struct shaped like
// the library's (heap arrays plus scalars, a free function that frees and nulls).  The free function must run exactly
// once per guard: on a normal exit, when an exception passes through the guard's scope, and when the struct was never
// filled.  ASan reports a double free or a leak; the counters catch a guard that does not call it.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "result_guard.h"

namespace {

struct fake_result {
    double* values;
    unsigned char* flags;
    unsigned long long count;
    double device_ms;
};
int g_free_calls = 0, g_freed_filled = 0;

void fake_result_free(fake_result* r) {
    if (!r) return;
    ++g_free_calls;
    if (r->values) ++g_freed_filled;
    std::free(r->values);
    std::free(r->flags);
    r->values = nullptr;
    r->flags = nullptr;
}
void fill(fake_result* r, unsigned long long n) {
    r->values = static_cast<double*>(std::calloc(n, sizeof(double)));
    r->flags = static_cast<unsigned char*>(std::calloc(n, 1));
    r->count = n;
    r->device_ms = 1.5;
}
using Guard = amchost::ResultGuard<fake_result, fake_result_free>;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            return 1;                                                          \
        }                                                                      \
    } while (0)

double use(bool fail) {
    Guard res;
    fill(res.get(), 64);
    if (fail) throw std::runtime_error("the apply step refused the result");
    return res->values[63] + res->device_ms;
}

}  // namespace

int main() {
    // a normal exit
    CHECK(use(false) == 1.5);
    CHECK(g_free_calls == 1 && g_freed_filled == 1);
    // an exception passes through the guard
    bool caught = false;
    try {
        use(true);
    } catch (const std::runtime_error&) {
        caught = true;
    }
    CHECK(caught && g_free_calls == 2 && g_freed_filled == 2);
    // the call that would have filled the struct threw first: the guard frees the zeroed struct, once
    caught = false;
    try {
        Guard res;
        CHECK(res->values == nullptr && res->flags == nullptr && res->count == 0);
        throw std::invalid_argument("the library refused the call");
    } catch (const std::invalid_argument&) {
        caught = true;
    }
    CHECK(caught && g_free_calls == 3 && g_freed_filled == 2);
    // the library freed its partial result itself before it returned the error: the second free finds nothing
    {
        Guard res;
        fill(res.get(), 8);
        fake_result_free(res.get());
    }
    CHECK(g_free_calls == 5 && g_freed_filled == 3);
    std::printf("result guard ok: %d free calls, %d of filled structs\n", g_free_calls, g_freed_filled);
    return 0;
}
