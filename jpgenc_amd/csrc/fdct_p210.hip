// K1 for P210 (10-bit 4:2:2 in 16-bit words: Y plane + interleaved Cb,Cr plane, a chroma row per pixel row): fdct.hip built with that load shape (see "input layouts" there).
#define JPGE_K1_SHAPE 14
#define JPGE_K1_ENTRY launch_fdct_p210
#include "fdct.hip"
