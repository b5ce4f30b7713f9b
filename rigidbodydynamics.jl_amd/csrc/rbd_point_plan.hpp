// rbd_point_plan.hpp — the host-side tables of rbd_workspace_set_points (rbd_point.hpp PointPlan): for every point the bodies of path(world → body), root
// first, and the union of those paths, parents first, with the points fixed to each of its bodies.  Plain C++: tests/test_point_kinematics_cpu.py compiles it.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rbd {

struct PointPlanTables {
  std::vector<int32_t> poff, path, uni, ubeg, upts;
};

// parent[b] < b for every body (the reference's order: rbd_model_create checks it), so ascending body index is parents first
inline PointPlanTables point_plan(int nb, const int32_t* parent, int np, const int32_t* body) {
  PointPlanTables P;
  P.poff.assign(1, 0);
  P.ubeg.assign(1, 0);
  std::vector<char> on((size_t)nb, 0);
  for (int k = 0; k < np; ++k) {
    const size_t p0 = P.path.size();
    for (int b = body[k]; b >= 0; b = parent[b]) { P.path.push_back(b); on[b] = 1; }
    std::reverse(P.path.begin() + p0, P.path.end());
    P.poff.push_back((int32_t)P.path.size());
  }
  for (int b = 0; b < nb; ++b) {
    if (!on[b]) continue;
    P.uni.push_back(b);
    for (int k = 0; k < np; ++k)
      if (body[k] == b) P.upts.push_back(k);
    P.ubeg.push_back((int32_t)P.upts.size());
  }
  return P;
}

}  // namespace rbd
