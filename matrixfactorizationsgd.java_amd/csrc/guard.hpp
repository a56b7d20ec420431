// guard.hpp -- the guard of the C-ABI: no C++ exception crosses the boundary (include/mfsgd.h).  Every `int` entry
// point runs its body in a wrapper over guard_run that reports where its unit reports: guarded() / guarded_free()
// (handle.hpp), dsgd_guarded() (dsgd.cpp), io_guarded() (io.cpp).
#pragma once

#include <string>

#include "../../include/mfsgd.h"

namespace mfsgd {

// std::bad_alloc becomes MFSGD_ERR_OOM, "out of host memory"; any other std::exception becomes `other`, what().
// `report` turns (code, what) into the return value; should even the message not fit into memory, the code goes back
// alone.
template <class F, class R>
int guard_run(F&& body, int other, R&& report) noexcept {
    int code = other;
    const char* what = "out of host memory";
    std::string kept;
    try {
        return body();
    } catch (const std::bad_alloc&) {
        code = MFSGD_ERR_OOM;
    } catch (const std::exception& e) {
        try {
            kept = e.what();
            what = kept.c_str();
        } catch (const std::exception&) {
            what = "";
        }
    }
    try {
        return report(code, what);
    } catch (const std::exception&) {
        return code;
    }
}

}  // namespace mfsgd
