// shapes.hpp — what the planner (plan.cpp, host only) and the wavefront kernels (wavefront.hpp,
// wavefront16.hpp) must agree on, one definition each.  No device code here.
#pragma once

namespace gx {

enum WfAlgo { WF_LOCAL = 0, WF_GLOBAL = 1, WF_SEMI = 2 };

constexpr int kWavesPerBlock = 4;

}  // namespace gx

// ---------------------------------------------------------------------------
// (G lanes per pair, R rows per lane) shapes: register-axis positions covered = G*R.  Each list
// is written once, here: the planner's arrays (plan.cpp kShapes / kShapes16) and every table
// of instances (wavefront16.hpp pick_instance) come from them.
//  * GX_SHAPES_R4: the int32 kernels (wavefront.hpp) and the packed kernels that store in groups
//    of 4 rows (traceback flags, band windows), R % 4 == 0;
//  * GX_SHAPES_PK: the packed score kernels (register axis = query for LOCAL/GLOBAL, target for
//    SEMI): R = 19 fits 150 bp (152 padded) and R = 23 fits 182 bp (184 padded) exactly; the
//    G = 16/32/64 shapes with few rows per lane serve small batches (make_plan).
// ---------------------------------------------------------------------------
#define GX_SHAPES_R4(X) X(8, 8) X(8, 12) X(8, 16) X(8, 20) X(16, 16) X(16, 20) X(32, 20) X(64, 20)
#define GX_SHAPES_PK(X)                                                                               \
    X(8, 8) X(8, 12) X(8, 16) X(8, 19) X(8, 20) X(8, 23) X(16, 10) X(16, 12) X(16, 16) X(16, 20)      \
    X(32, 5) X(32, 6) X(32, 9) X(32, 20) X(64, 3) X(64, 5) X(64, 20)
