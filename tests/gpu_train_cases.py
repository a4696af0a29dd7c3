"""The cases of tests/test_gpu_shape_decoder_train.py: (B, T, Z, L, loss_type, seed) and the chunk sizes each runs with, in
units of the training tile (0 = the library's default: one chunk here).  The seeds are chosen on the CPU so that at most 1/8 of a
case's points are fragile (tests/test_shape_decoder_train_cpu.py asserts it from the float64 oracle alone).

Why these shapes: the smallest at which the kernels take another path.  One point; one below, at and above the tile of 128; one
below, at and above a chunk of two tiles; three chunks with a ragged last one; B = 3 with T no multiple of 16, so that 16-point
groups and tiles mix shapes and a shape's points span chunks; the depth limits 1 and 8; the latent limits 1 and 256; occupancy."""
TILE = 128                                                 # shapemol_field_train_tile (the GPU test reads it from the library)

# (B, T, Z, L, loss_type, seed): chunk sizes in tiles
CASES = {
    (1, 1, 32, 4, "signeddist", 301): (0,),
    (1, TILE - 1, 32, 4, "signeddist", 302): (0,),
    (1, TILE, 32, 4, "signeddist", 303): (0,),
    (1, TILE + 1, 32, 4, "signeddist", 304): (0, 2),
    (1, 2 * TILE - 1, 32, 4, "signeddist", 305): (2,),
    (1, 2 * TILE, 32, 4, "signeddist", 306): (2,),
    (1, 2 * TILE + 1, 32, 4, "signeddist", 307): (2,),
    (3, 183, 32, 4, "signeddist", 308): (0, 2),            # 549 points: chunks of 256, 256, 37
    (3, 183, 32, 4, "occupancy", 309): (0, 2),
    (2, 77, 32, 1, "signeddist", 310): (0,),
    (2, 77, 32, 8, "signeddist", 311): (0, 1),
    (2, 77, 1, 4, "signeddist", 312): (0,),
    (2, 77, 256, 4, "occupancy", 313): (0,),
}

# More tiles than workgroups: a workgroup strides over several tiles of one chunk only when a caller asks for a chunk above the
# default of one tile per compute unit.  CUS compute units (an MI355X has 256), one chunk of CUS + 1 tiles (the smallest that strides), the last tile one point; one block, to keep the float64 oracle quick.
CUS = 256
STRIDE_CASE = (1, CUS * TILE + 1, 32, 1, "signeddist", 314)
STRIDE_CHUNK_TILES = CUS + 1


def all_cases():
    return list(CASES)
