// K1 for I420 (Y, Cb, Cr planes, chroma at half size): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 5
#define JPGE_K1_ENTRY launch_fdct_i420
#include "fdct.hip"
