// result_guard.h — a scope guard for the library's amc_*_result structs: it holds the struct, zero-initialised, and calls
// the matching amc_*_result_free when the scope ends, by return or by exception.  Every such free function takes a
// zeroed or already freed struct (it frees null pointers and nulls what it freed), so the guard may be declared before
// the call that fills it.  No pybind11 here: tests/shim/result_guard_check.cc compiles this header on its own.
#pragma once

namespace amchost {

template <typename Result, void (*Free)(Result*)>
class ResultGuard {
  public:
    ResultGuard() = default;
    ResultGuard(const ResultGuard&) = delete;
    ResultGuard& operator=(const ResultGuard&) = delete;
    ~ResultGuard() { Free(&res_); }
    Result* get() { return &res_; }  // for the library call that fills it
    const Result* operator->() const { return &res_; }

  private:
    Result res_{};
};

}  // namespace amchost
