// semi_tb.hip — the direction-flag kernels of gasalx_semi_cigar_* (SEMI-GLOBAL, HEAD = TAIL =
// TARGET): the packed WF16_SEMI_TB instances (wavefront16.hpp) over the traceback shapes
// (R % 4 == 0), and the int32 kernel with traceback words under the same boundary
// (wavefront.hpp, SEMITB) for the blocks the packed launch declines or the value window
// refuses; and the same two families under the boundary of any HEAD for gasalx_semi_cigar_head_*
// (WF16_SEMI_TBH, SEMITB = 2: the head is a kernel argument).  Compiled apart from dispatch.hip so the two build in parallel and dispatch.hip's
// own instances are not touched.
#include "wavefront16.hpp"

namespace gx {

struct StbK {
    template <int G, int R> static Wf16Fn fn() { return &wf16_kernel<WF16_SEMI_TB, G, R>; }
};
struct StbK32 {
    template <int G, int R> static Wf16Fn fn() { return &wf_semi_tb_kernel<G, R>; }
};

struct SthK {
    template <int G, int R> static Wf16Fn fn() { return &wf16_kernel<WF16_SEMI_TBH, G, R>; }
};
struct SthK32 {
    template <int G, int R> static Wf16Fn fn() { return &wf_semi_tb_kernel<G, R, true>; }
};

Wf16Fn wf16_semi_tb_lookup(int G, int R, bool heads) {
    return heads ? pick_instance<SthK, SHAPES_R4>(G, R) : pick_instance<StbK, SHAPES_R4>(G, R);
}
Wf16Fn wf_semi_tb_lookup(int G, int R, bool heads) {
    return heads ? pick_instance<SthK32, SHAPES_R4>(G, R) : pick_instance<StbK32, SHAPES_R4>(G, R);
}

}  // namespace gx
