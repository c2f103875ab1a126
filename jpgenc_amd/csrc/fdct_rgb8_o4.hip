// K1 for RGB8, oriented, transposed and mirrored (JPGE_ORIENT_TRANSVERSE, _ROT270): fdct.hip built with that load shape and orientation class (see "oriented loads" there).
#define JPGE_K1_SHAPE 0
#define JPGE_K1_ORIENT 4
#define JPGE_K1_ENTRY launch_fdct_rgb8_o4
#include "fdct.hip"
