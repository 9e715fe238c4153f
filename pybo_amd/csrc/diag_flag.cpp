// diag_flag.cpp -- the one object in which libgpx.so and libgpx_diag.so differ (build.sh compiles it twice, the second time
// with -DGPX_DIAGNOSTICS): whether gpx_set_option accepts the diagnostic options of gpx_diag.h.  Every other object is shared.
#include "../../include/gpx.h"

extern "C" int gpx_diagnostics(void) {
#ifdef GPX_DIAGNOSTICS
    return 1;
#else
    return 0;
#endif
}
