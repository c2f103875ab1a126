// K1 for RGB8, oriented, mirrored (JPGE_ORIENT_FLIP_H, _ROT180): fdct.hip built with that load shape and orientation class (see "oriented loads" there).
#define JPGE_K1_SHAPE 0
#define JPGE_K1_ORIENT 2
#define JPGE_K1_ENTRY launch_fdct_rgb8_o2
#include "fdct.hip"
