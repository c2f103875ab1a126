// K1 for NV12 (Y plane + interleaved Cb,Cr plane at half size): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 4
#define JPGE_K1_ENTRY launch_fdct_nv12
#include "fdct.hip"
