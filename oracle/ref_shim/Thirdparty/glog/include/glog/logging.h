// Stand-in for glog, reached through the relative path the reference's include/gyro_aided_tracker.h writes
// ("../Thirdparty/glog/include/glog/logging.h", resolved against oracle/ref_shim/tracker on the include path).
// TEST INFRASTRUCTURE (oracle/README.md).  LOG(severity) swallows whatever is streamed into it.
#ifndef PAGK_REF_SHIM_GLOG_LOGGING_H
#define PAGK_REF_SHIM_GLOG_LOGGING_H

#include <ostream>

namespace pagk_ref_shim {
struct NullStream {
    template <typename T> NullStream &operator<<(const T &) { return *this; }
    NullStream &operator<<(std::ostream &(*)(std::ostream &)) { return *this; }
};
}   // namespace pagk_ref_shim

#define LOG(severity) pagk_ref_shim::NullStream()

#endif
