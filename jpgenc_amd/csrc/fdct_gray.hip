// K1 for one plane of 8-bit luminance (GRAY8): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 7
#define JPGE_K1_ENTRY launch_fdct_gray
#include "fdct.hip"
