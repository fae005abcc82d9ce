// K3's semantic masks (tds_raster_scene_masks, tds_raster_scene_masks_multi; include/tdship.h): raster.hip once more, with only the mask
// entry points and their launches.  The bit-plane kernels instantiated with the mask tags (MaskU8, MaskBits) so live in a code object of their
// own, and every colour kernel of raster.hip keeps its code byte for byte (a kernel added to raster.hip's code object moves the data its code
// addresses relative to the program counter).
#define TDS_RASTER_MASKS_TU
#include "raster.hip"
