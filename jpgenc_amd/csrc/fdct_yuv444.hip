// K1 for planar Y, Cb, Cr at full size (YUV444_PLANAR): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 6
#define JPGE_K1_ENTRY launch_fdct_yuv444
#include "fdct.hip"
