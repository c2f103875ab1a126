// K1 for 8-bit Bayer mosaics (RGGB, GRBG, GBRG, BGGR; bilinear demosaic in the staging): fdct.hip built with that load shape (see "Bayer loads" there).
#define JPGE_K1_SHAPE 17
#define JPGE_K1_ENTRY launch_fdct_bayer8
#include "fdct.hip"
