// local_rs.hip — instances of the packed LOCAL e-drift kernel (wavefront16.hpp) with u16 keys
// (WF16_LOCAL_U16) and the WITH_START reverse pass's early stop (WF16_LOCAL_RS,
// WF16_LOCAL_U16_RS) and with keys by step segments (WF16_LOCAL_SEG), over the packed shapes
// (shapes.hpp GX_SHAPES_PK).  Compiled apart from dispatch.hip so the two build in parallel.
#include "wavefront16.hpp"

namespace gx {

template <int ALGO>
static Wf16Fn pick_pk(int G, int R) { return pick_instance<Wf16K<ALGO>, SHAPES_PK>(G, R); }

Wf16Fn wf16_local_lookup(int G, int R, bool u16, bool rs, bool seg) {
    if (seg) return pick_pk<WF16_LOCAL_SEG>(G, R);
    if (rs) return u16 ? pick_pk<WF16_LOCAL_U16_RS>(G, R) : pick_pk<WF16_LOCAL_RS>(G, R);
    return u16 ? pick_pk<WF16_LOCAL_U16>(G, R) : pick_pk<WF_LOCAL>(G, R);
}

}  // namespace gx
