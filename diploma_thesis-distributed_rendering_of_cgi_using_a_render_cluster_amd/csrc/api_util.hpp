// What every file behind the C ABI (rr_api.cpp, rr_debug.cpp, frame.cpp,
// coders.cpp) shares: the thread's error string, the exception barrier, clocks.
#pragma once

#include <chrono>
#include <new>
#include <string>

#include "device.hpp"
#include "rr.h"

namespace rr {

inline thread_local std::string g_err;  // rr_last_error
inline thread_local std::string g_warn;  // rr_last_warning(NULL): the thread's last host encode (rr_encode_image)

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// Catch-all wrapper: C++ exceptions never cross the C ABI.
template <typename F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const HipError& e) {
        return fail(RR_ENODEV, e.what());
    } catch (const std::bad_alloc&) {
        return fail(RR_ENOMEM, "out of host memory");
    } catch (const std::exception& e) {
        return fail(RR_EINVAL, e.what());
    }
}

inline double unix_now() {
    using namespace std::chrono;
    return duration_cast<duration<double>>(system_clock::now().time_since_epoch()).count();
}

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace rr
