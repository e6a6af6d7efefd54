// unseen_report.h -- the report of unseen branches as the generated source writes it (device/unseen.hip behind GFH_UNSEEN_CAP,
// emit_branching.cpp) and the host reads it (passes.cpp, recover_unseen): from byte 128 of the status area up to kUnseenCap entries.
#pragma once

namespace gfh {

constexpr int kUnseenCap = 120;
struct UnseenEntry { long long slot; unsigned long long path; int n_guards; int pad; };      // = struct gfh_unseen of unseen.hip

}  // namespace gfh
