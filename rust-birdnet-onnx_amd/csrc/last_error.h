// The one declaration of the C ABI's error report, for translation units with the runtime (through capi_internal.h) and without it
// (index_file.cpp).  Defined in capi.cpp; a stand-alone program over host-only code defines its own (tools/asan_index_file.cpp).
#pragma once
#include <string>

#include "../../include/birdnet_hip.h"

namespace bn {
// sets the message bn_last_error() returns on this thread; returns st
bn_status set_last_error(bn_status st, const std::string &msg);
}  // namespace bn
