// K1 for I010 (10-bit 4:2:0 in 16-bit words: Y, Cb, Cr planes, chroma at half size): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 12
#define JPGE_K1_ENTRY launch_fdct_i010
#include "fdct.hip"
