// K1 for interleaved B,G,R (BGR8): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 1
#define JPGE_K1_ENTRY launch_fdct_bgr8
#include "fdct.hip"
