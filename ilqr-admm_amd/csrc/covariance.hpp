// covariance.hpp -- launch wrapper of isls_cov_closed_loop_* (csrc/covariance.hip), declared apart from isls_common.hpp: that
// header is also read by the run-time compiler of user models and costs, which has no use for this host-side entry point.
#pragma once
#include "isls_common.hpp"

namespace isls {

template <typename T> int launch_cov_closed_loop(const isls_cov_args &a, hipStream_t s);

}  // namespace isls
