// The "bf16x3" (three-term split) instantiations of the bf16 convolution kernel: see tpspp_conv_bf16.hip / _impl.h.
#include "tpspp_conv_bf16_impl.h"

namespace tpspp {

int conv_bf16x3_launch(const BParams& P, const BRoute& R, hipStream_t st)
{
    bool ok = false;
    if (R.kh == 1 && R.sh == 1 && R.sw == 1)      ok = launch_by_shape<1, 1, 1, kKC1, true>(P, R, st);
    else if (R.kh == 1 && R.sh == 2 && R.sw == 2) ok = launch_by_shape<1, 2, 2, kKC1, true>(P, R, st);
    else if (R.kh == 3 && R.sh == 1 && R.sw == 1) ok = launch_by_shape<3, 1, 1, kKC3, true>(P, R, st);
    else if (R.kh == 3 && R.sh == 2 && R.sw == 2) ok = launch_by_shape<3, 2, 2, kKC3, true>(P, R, st);
    else if (R.kh == 3 && R.sh == 2 && R.sw == 1) ok = launch_by_shape<3, 2, 1, kKC3, true>(P, R, st);
    TPSPP_REQUIRE(ok, "tpspp_conv2d_bf16_fwd(tiled-x3): the route names no kernel");
    return TPSPP_OK;
}

}  // namespace tpspp
