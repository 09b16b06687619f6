"""CPU restatement of the mesh-export pipeline (sparsefusion_amd/mesh.py) for the tests.

* `marching_cubes(vol, iso)`: float32 / numpy marching cubes that produces the library's canonical output order, with its own copy
  of the Lorensen / Bourke tables (classic numbering 0 (0,0,0) 1 (1,0,0) 2 (1,1,0) 3 (0,1,0) 4 (0,0,1) 5 (1,0,1) 6 (1,1,1) 7 (0,1,1)):
    - a corner is inside when v < iso (fp32 compare);
    - vertex ids: point-major in x-major order (p = (i * ny + j) * nz + k), then axis x < y < z of the point's owned edge toward
      +axis; the vertex sits at a + t along that axis, t = (iso - v_a) / (v_b - v_a) in fp32;
    - faces: cell x-major order, then triangle order within the table row, corners in table order -- with inside = v < iso the
      table's winding makes faces look toward decreasing field values (outward on a density blob).
* `smooth_gaussian(vol, sigma)`: PyMCubes' definition, scipy.ndimage.gaussian_filter(float64(vol) - 0.5, sigma).
* `iso_level(vol)`: the reference export's level, mean + 0.25 * std (numpy float64, ddof 0).

PyMCubes itself is not available, so parity with its vertex order, welding and winding is not pinned; this file pins the library's
own canonical order."""
import numpy as np

# edges as (corner a, corner b) of the classic numbering
EDGE_CORNERS = ((0, 1), (1, 2), (3, 2), (0, 3), (4, 5), (5, 6), (7, 6), (4, 7), (0, 4), (1, 5), (2, 6), (3, 7))
CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
# edge -> (owner point offset (dx, dy, dz), axis): the lower corner of the edge owns it
EDGE_OWNER = tuple((CORNERS[a], [CORNERS[b][d] - CORNERS[a][d] for d in range(3)].index(1)) for a, b in EDGE_CORNERS)

TRI_TABLE = (
    (), (0, 8, 3), (0, 1, 9), (1, 8, 3, 9, 8, 1), (1, 2, 10), (0, 8, 3, 1, 2, 10), (9, 2, 10, 0, 2, 9),
    (2, 8, 3, 2, 10, 8, 10, 9, 8), (3, 11, 2), (0, 11, 2, 8, 11, 0), (1, 9, 0, 2, 3, 11), (1, 11, 2, 1, 9, 11, 9, 8, 11),
    (3, 10, 1, 11, 10, 3), (0, 10, 1, 0, 8, 10, 8, 11, 10), (3, 9, 0, 3, 11, 9, 11, 10, 9), (9, 8, 10, 10, 8, 11),
    (4, 7, 8), (4, 3, 0, 7, 3, 4), (0, 1, 9, 8, 4, 7), (4, 1, 9, 4, 7, 1, 7, 3, 1), (1, 2, 10, 8, 4, 7),
    (3, 4, 7, 3, 0, 4, 1, 2, 10), (9, 2, 10, 9, 0, 2, 8, 4, 7), (2, 10, 9, 2, 9, 7, 2, 7, 3, 7, 9, 4), (8, 4, 7, 3, 11, 2),
    (11, 4, 7, 11, 2, 4, 2, 0, 4), (9, 0, 1, 8, 4, 7, 2, 3, 11), (4, 7, 11, 9, 4, 11, 9, 11, 2, 9, 2, 1),
    (3, 10, 1, 3, 11, 10, 7, 8, 4), (1, 11, 10, 1, 4, 11, 1, 0, 4, 7, 11, 4), (4, 7, 8, 9, 0, 11, 9, 11, 10, 11, 0, 3),
    (4, 7, 11, 4, 11, 9, 9, 11, 10), (9, 5, 4), (9, 5, 4, 0, 8, 3), (0, 5, 4, 1, 5, 0), (8, 5, 4, 8, 3, 5, 3, 1, 5),
    (1, 2, 10, 9, 5, 4), (3, 0, 8, 1, 2, 10, 4, 9, 5), (5, 2, 10, 5, 4, 2, 4, 0, 2), (2, 10, 5, 3, 2, 5, 3, 5, 4, 3, 4, 8),
    (9, 5, 4, 2, 3, 11), (0, 11, 2, 0, 8, 11, 4, 9, 5), (0, 5, 4, 0, 1, 5, 2, 3, 11), (2, 1, 5, 2, 5, 8, 2, 8, 11, 4, 8, 5),
    (10, 3, 11, 10, 1, 3, 9, 5, 4), (4, 9, 5, 0, 8, 1, 8, 10, 1, 8, 11, 10), (5, 4, 0, 5, 0, 11, 5, 11, 10, 11, 0, 3),
    (5, 4, 8, 5, 8, 10, 10, 8, 11), (9, 7, 8, 5, 7, 9), (9, 3, 0, 9, 5, 3, 5, 7, 3), (0, 7, 8, 0, 1, 7, 1, 5, 7),
    (1, 5, 3, 3, 5, 7), (9, 7, 8, 9, 5, 7, 10, 1, 2), (10, 1, 2, 9, 5, 0, 5, 3, 0, 5, 7, 3),
    (8, 0, 2, 8, 2, 5, 8, 5, 7, 10, 5, 2), (2, 10, 5, 2, 5, 3, 3, 5, 7), (7, 9, 5, 7, 8, 9, 3, 11, 2),
    (9, 5, 7, 9, 7, 2, 9, 2, 0, 2, 7, 11), (2, 3, 11, 0, 1, 8, 1, 7, 8, 1, 5, 7), (11, 2, 1, 11, 1, 7, 7, 1, 5),
    (9, 5, 8, 8, 5, 7, 10, 1, 3, 10, 3, 11), (5, 7, 0, 5, 0, 9, 7, 11, 0, 1, 0, 10, 11, 10, 0),
    (11, 10, 0, 11, 0, 3, 10, 5, 0, 8, 0, 7, 5, 7, 0), (11, 10, 5, 7, 11, 5), (10, 6, 5), (0, 8, 3, 5, 10, 6),
    (9, 0, 1, 5, 10, 6), (1, 8, 3, 1, 9, 8, 5, 10, 6), (1, 6, 5, 2, 6, 1), (1, 6, 5, 1, 2, 6, 3, 0, 8),
    (9, 6, 5, 9, 0, 6, 0, 2, 6), (5, 9, 8, 5, 8, 2, 5, 2, 6, 3, 2, 8), (2, 3, 11, 10, 6, 5), (11, 0, 8, 11, 2, 0, 10, 6, 5),
    (0, 1, 9, 2, 3, 11, 5, 10, 6), (5, 10, 6, 1, 9, 2, 9, 11, 2, 9, 8, 11), (6, 3, 11, 6, 5, 3, 5, 1, 3),
    (0, 8, 11, 0, 11, 5, 0, 5, 1, 5, 11, 6), (3, 11, 6, 0, 3, 6, 0, 6, 5, 0, 5, 9), (6, 5, 9, 6, 9, 11, 11, 9, 8),
    (5, 10, 6, 4, 7, 8), (4, 3, 0, 4, 7, 3, 6, 5, 10), (1, 9, 0, 5, 10, 6, 8, 4, 7), (10, 6, 5, 1, 9, 7, 1, 7, 3, 7, 9, 4),
    (6, 1, 2, 6, 5, 1, 4, 7, 8), (1, 2, 5, 5, 2, 6, 3, 0, 4, 3, 4, 7), (8, 4, 7, 9, 0, 5, 0, 6, 5, 0, 2, 6),
    (7, 3, 9, 7, 9, 4, 3, 2, 9, 5, 9, 6, 2, 6, 9), (3, 11, 2, 7, 8, 4, 10, 6, 5), (5, 10, 6, 4, 7, 2, 4, 2, 0, 2, 7, 11),
    (0, 1, 9, 4, 7, 8, 2, 3, 11, 5, 10, 6), (9, 2, 1, 9, 11, 2, 9, 4, 11, 7, 11, 4, 5, 10, 6),
    (8, 4, 7, 3, 11, 5, 3, 5, 1, 5, 11, 6), (5, 1, 11, 5, 11, 6, 1, 0, 11, 7, 11, 4, 0, 4, 11),
    (0, 5, 9, 0, 6, 5, 0, 3, 6, 11, 6, 3, 8, 4, 7), (6, 5, 9, 6, 9, 11, 4, 7, 9, 7, 11, 9), (10, 4, 9, 6, 4, 10),
    (4, 10, 6, 4, 9, 10, 0, 8, 3), (10, 0, 1, 10, 6, 0, 6, 4, 0), (8, 3, 1, 8, 1, 6, 8, 6, 4, 6, 1, 10),
    (1, 4, 9, 1, 2, 4, 2, 6, 4), (3, 0, 8, 1, 2, 9, 2, 4, 9, 2, 6, 4), (0, 2, 4, 4, 2, 6), (8, 3, 2, 8, 2, 4, 4, 2, 6),
    (10, 4, 9, 10, 6, 4, 11, 2, 3), (0, 8, 2, 2, 8, 11, 4, 9, 10, 4, 10, 6), (3, 11, 2, 0, 1, 6, 0, 6, 4, 6, 1, 10),
    (6, 4, 1, 6, 1, 10, 4, 8, 1, 2, 1, 11, 8, 11, 1), (9, 6, 4, 9, 3, 6, 9, 1, 3, 11, 6, 3),
    (8, 11, 1, 8, 1, 0, 11, 6, 1, 9, 1, 4, 6, 4, 1), (3, 11, 6, 3, 6, 0, 0, 6, 4), (6, 4, 8, 11, 6, 8),
    (7, 10, 6, 7, 8, 10, 8, 9, 10), (0, 7, 3, 0, 10, 7, 0, 9, 10, 6, 7, 10), (10, 6, 7, 1, 10, 7, 1, 7, 8, 1, 8, 0),
    (10, 6, 7, 10, 7, 1, 1, 7, 3), (1, 2, 6, 1, 6, 8, 1, 8, 9, 8, 6, 7), (2, 6, 9, 2, 9, 1, 6, 7, 9, 0, 9, 3, 7, 3, 9),
    (7, 8, 0, 7, 0, 6, 6, 0, 2), (7, 3, 2, 6, 7, 2), (2, 3, 11, 10, 6, 8, 10, 8, 9, 8, 6, 7),
    (2, 0, 7, 2, 7, 11, 0, 9, 7, 6, 7, 10, 9, 10, 7), (1, 8, 0, 1, 7, 8, 1, 10, 7, 6, 7, 10, 2, 3, 11),
    (11, 2, 1, 11, 1, 7, 10, 6, 1, 6, 7, 1), (8, 9, 6, 8, 6, 7, 9, 1, 6, 11, 6, 3, 1, 3, 6), (0, 9, 1, 11, 6, 7),
    (7, 8, 0, 7, 0, 6, 3, 11, 0, 11, 6, 0), (7, 11, 6), (7, 6, 11), (3, 0, 8, 11, 7, 6), (0, 1, 9, 11, 7, 6),
    (8, 1, 9, 8, 3, 1, 11, 7, 6), (10, 1, 2, 6, 11, 7), (1, 2, 10, 3, 0, 8, 6, 11, 7), (2, 9, 0, 2, 10, 9, 6, 11, 7),
    (6, 11, 7, 2, 10, 3, 10, 8, 3, 10, 9, 8), (7, 2, 3, 6, 2, 7), (7, 0, 8, 7, 6, 0, 6, 2, 0), (2, 7, 6, 2, 3, 7, 0, 1, 9),
    (1, 6, 2, 1, 8, 6, 1, 9, 8, 8, 7, 6), (10, 7, 6, 10, 1, 7, 1, 3, 7), (10, 7, 6, 1, 7, 10, 1, 8, 7, 1, 0, 8),
    (0, 3, 7, 0, 7, 10, 0, 10, 9, 6, 10, 7), (7, 6, 10, 7, 10, 8, 8, 10, 9), (6, 8, 4, 11, 8, 6), (3, 6, 11, 3, 0, 6, 0, 4, 6),
    (8, 6, 11, 8, 4, 6, 9, 0, 1), (9, 4, 6, 9, 6, 3, 9, 3, 1, 11, 3, 6), (6, 8, 4, 6, 11, 8, 2, 10, 1),
    (1, 2, 10, 3, 0, 11, 0, 6, 11, 0, 4, 6), (4, 11, 8, 4, 6, 11, 0, 2, 9, 2, 10, 9),
    (10, 9, 3, 10, 3, 2, 9, 4, 3, 11, 3, 6, 4, 6, 3), (8, 2, 3, 8, 4, 2, 4, 6, 2), (0, 4, 2, 4, 6, 2),
    (1, 9, 0, 2, 3, 4, 2, 4, 6, 4, 3, 8), (1, 9, 4, 1, 4, 2, 2, 4, 6), (8, 1, 3, 8, 6, 1, 8, 4, 6, 6, 10, 1),
    (10, 1, 0, 10, 0, 6, 6, 0, 4), (4, 6, 3, 4, 3, 8, 6, 10, 3, 0, 3, 9, 10, 9, 3), (10, 9, 4, 6, 10, 4), (4, 9, 5, 7, 6, 11),
    (0, 8, 3, 4, 9, 5, 11, 7, 6), (5, 0, 1, 5, 4, 0, 7, 6, 11), (11, 7, 6, 8, 3, 4, 3, 5, 4, 3, 1, 5),
    (9, 5, 4, 10, 1, 2, 7, 6, 11), (6, 11, 7, 1, 2, 10, 0, 8, 3, 4, 9, 5), (7, 6, 11, 5, 4, 10, 4, 2, 10, 4, 0, 2),
    (3, 4, 8, 3, 5, 4, 3, 2, 5, 10, 5, 2, 11, 7, 6), (7, 2, 3, 7, 6, 2, 5, 4, 9), (9, 5, 4, 0, 8, 6, 0, 6, 2, 6, 8, 7),
    (3, 6, 2, 3, 7, 6, 1, 5, 0, 5, 4, 0), (6, 2, 8, 6, 8, 7, 2, 1, 8, 4, 8, 5, 1, 5, 8), (9, 5, 4, 10, 1, 6, 1, 7, 6, 1, 3, 7),
    (1, 6, 10, 1, 7, 6, 1, 0, 7, 8, 7, 0, 9, 5, 4), (4, 0, 10, 4, 10, 5, 0, 3, 10, 6, 10, 7, 3, 7, 10),
    (7, 6, 10, 7, 10, 8, 5, 4, 10, 4, 8, 10), (6, 9, 5, 6, 11, 9, 11, 8, 9), (3, 6, 11, 0, 6, 3, 0, 5, 6, 0, 9, 5),
    (0, 11, 8, 0, 5, 11, 0, 1, 5, 5, 6, 11), (6, 11, 3, 6, 3, 5, 5, 3, 1), (1, 2, 10, 9, 5, 11, 9, 11, 8, 11, 5, 6),
    (0, 11, 3, 0, 6, 11, 0, 9, 6, 5, 6, 9, 1, 2, 10), (11, 8, 5, 11, 5, 6, 8, 0, 5, 10, 5, 2, 0, 2, 5),
    (6, 11, 3, 6, 3, 5, 2, 10, 3, 10, 5, 3), (5, 8, 9, 5, 2, 8, 5, 6, 2, 3, 8, 2), (9, 5, 6, 9, 6, 0, 0, 6, 2),
    (1, 5, 8, 1, 8, 0, 5, 6, 8, 3, 8, 2, 6, 2, 8), (1, 5, 6, 2, 1, 6), (1, 3, 6, 1, 6, 10, 3, 8, 6, 5, 6, 9, 8, 9, 6),
    (10, 1, 0, 10, 0, 6, 9, 5, 0, 5, 6, 0), (0, 3, 8, 5, 6, 10), (10, 5, 6), (11, 5, 10, 7, 5, 11),
    (11, 5, 10, 11, 7, 5, 8, 3, 0), (5, 11, 7, 5, 10, 11, 1, 9, 0), (10, 7, 5, 10, 11, 7, 9, 8, 1, 8, 3, 1),
    (11, 1, 2, 11, 7, 1, 7, 5, 1), (0, 8, 3, 1, 2, 7, 1, 7, 5, 7, 2, 11), (9, 7, 5, 9, 2, 7, 9, 0, 2, 2, 11, 7),
    (7, 5, 2, 7, 2, 11, 5, 9, 2, 3, 2, 8, 9, 8, 2), (2, 5, 10, 2, 3, 5, 3, 7, 5), (8, 2, 0, 8, 5, 2, 8, 7, 5, 10, 2, 5),
    (9, 0, 1, 5, 10, 3, 5, 3, 7, 3, 10, 2), (9, 8, 2, 9, 2, 1, 8, 7, 2, 10, 2, 5, 7, 5, 2), (1, 3, 5, 3, 7, 5),
    (0, 8, 7, 0, 7, 1, 1, 7, 5), (9, 0, 3, 9, 3, 5, 5, 3, 7), (9, 8, 7, 5, 9, 7), (5, 8, 4, 5, 10, 8, 10, 11, 8),
    (5, 0, 4, 5, 11, 0, 5, 10, 11, 11, 3, 0), (0, 1, 9, 8, 4, 10, 8, 10, 11, 10, 4, 5),
    (10, 11, 4, 10, 4, 5, 11, 3, 4, 9, 4, 1, 3, 1, 4), (2, 5, 1, 2, 8, 5, 2, 11, 8, 4, 5, 8),
    (0, 4, 11, 0, 11, 3, 4, 5, 11, 2, 11, 1, 5, 1, 11), (0, 2, 5, 0, 5, 9, 2, 11, 5, 4, 5, 8, 11, 8, 5), (9, 4, 5, 2, 11, 3),
    (2, 5, 10, 3, 5, 2, 3, 4, 5, 3, 8, 4), (5, 10, 2, 5, 2, 4, 4, 2, 0), (3, 10, 2, 3, 5, 10, 3, 8, 5, 4, 5, 8, 0, 1, 9),
    (5, 10, 2, 5, 2, 4, 1, 9, 2, 9, 4, 2), (8, 4, 5, 8, 5, 3, 3, 5, 1), (0, 4, 5, 1, 0, 5), (8, 4, 5, 8, 5, 3, 9, 0, 5, 0, 3, 5),
    (9, 4, 5), (4, 11, 7, 4, 9, 11, 9, 10, 11), (0, 8, 3, 4, 9, 7, 9, 11, 7, 9, 10, 11), (1, 10, 11, 1, 11, 4, 1, 4, 0, 7, 4, 11),
    (3, 1, 4, 3, 4, 8, 1, 10, 4, 7, 4, 11, 10, 11, 4), (4, 11, 7, 9, 11, 4, 9, 2, 11, 9, 1, 2),
    (9, 7, 4, 9, 11, 7, 9, 1, 11, 2, 11, 1, 0, 8, 3), (11, 7, 4, 11, 4, 2, 2, 4, 0), (11, 7, 4, 11, 4, 2, 8, 3, 4, 3, 2, 4),
    (2, 9, 10, 2, 7, 9, 2, 3, 7, 7, 4, 9), (9, 10, 7, 9, 7, 4, 10, 2, 7, 8, 7, 0, 2, 0, 7),
    (3, 7, 10, 3, 10, 2, 7, 4, 10, 1, 10, 0, 4, 0, 10), (1, 10, 2, 8, 7, 4), (4, 9, 1, 4, 1, 7, 7, 1, 3),
    (4, 9, 1, 4, 1, 7, 0, 8, 1, 8, 7, 1), (4, 0, 3, 7, 4, 3), (4, 8, 7), (9, 10, 8, 10, 11, 8), (3, 0, 9, 3, 9, 11, 11, 9, 10),
    (0, 1, 10, 0, 10, 8, 8, 10, 11), (3, 1, 10, 11, 3, 10), (1, 2, 11, 1, 11, 9, 9, 11, 8), (3, 0, 9, 3, 9, 11, 1, 2, 9, 2, 11, 9),
    (0, 2, 11, 8, 0, 11), (3, 2, 11), (2, 3, 8, 2, 8, 10, 10, 8, 9), (9, 10, 2, 0, 9, 2), (2, 3, 8, 2, 8, 10, 0, 1, 8, 1, 10, 8),
    (1, 10, 2), (1, 3, 8, 9, 1, 8), (0, 9, 1), (0, 3, 8), (),
)
assert len(TRI_TABLE) == 256 and all(len(r) % 3 == 0 and len(r) <= 15 for r in TRI_TABLE)


def crossing_edges(case):
    """Edges whose two corners classify differently in cube configuration `case` (bit c set = corner c inside)."""
    return {e for e, (a, b) in enumerate(EDGE_CORNERS) if ((case >> a) ^ (case >> b)) & 1}


def edge_table():
    """The 256-entry edge table: bit e set when edge e crosses."""
    return [sum(1 << e for e in crossing_edges(c)) for c in range(256)]


def marching_cubes(vol, iso):
    """vol [nx, ny, nz] float32, iso float32 -> (vertices [V, 3] float32 in index coordinates, faces [F, 3] int32), canonical order."""
    v = np.ascontiguousarray(vol, dtype=np.float32)
    iso = np.float32(iso)
    nx, ny, nz = v.shape
    inside = v < iso
    N = v.size
    flat = v.reshape(-1)
    strides = (ny * nz, nz, 1)
    # owned crossing edges of every point, flattened point-major then axis
    cross = np.zeros((N, 3), dtype=bool)
    for a in range(3):
        sl = [slice(None)] * 3
        sl[a] = slice(0, v.shape[a] - 1)
        sh = [slice(None)] * 3
        sh[a] = slice(1, None)
        c = np.zeros(v.shape, dtype=bool)
        c[tuple(sl)] = inside[tuple(sl)] != inside[tuple(sh)]
        cross[:, a] = c.reshape(-1)
    vid = np.cumsum(cross.reshape(-1)) - 1
    vid = vid.reshape(N, 3).astype(np.int64)
    p, ax = np.nonzero(cross)
    va = flat[p]
    vb = flat[p + np.asarray(strides, dtype=np.int64)[ax]]
    t = (iso - va) / (vb - va)                                     # fp32, one rounding per operation
    idx = np.stack(np.unravel_index(p, v.shape), axis=1).astype(np.float32)
    idx[np.arange(p.size), ax] = idx[np.arange(p.size), ax] + t.astype(np.float32)
    verts = idx.astype(np.float32)
    # cells
    if min(nx, ny, nz) < 2:
        return verts, np.zeros((0, 3), dtype=np.int32)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int32)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int32) << c
    ci, cj, ck = np.nonzero(case)                                 # x-major cell order (np.nonzero is C order)
    cases = case[ci, cj, ck]
    cell_p = (ci * ny + cj) * nz + ck
    ntri = np.array([len(r) // 3 for r in TRI_TABLE])[cases]
    table = np.full((256, 15), -1, dtype=np.int64)
    for c, r in enumerate(TRI_TABLE):
        table[c, :len(r)] = r
    owner_off = np.array([(dx * ny + dy) * nz + dz for (dx, dy, dz), _ in EDGE_OWNER], dtype=np.int64)
    owner_ax = np.array([a for _, a in EDGE_OWNER], dtype=np.int64)
    faces, keys = [], []
    for s in range(5):
        m = ntri > s
        e = table[cases[m], 3 * s:3 * s + 3]                      # [n, 3] edges
        ids = vid[cell_p[m][:, None] + owner_off[e], owner_ax[e]]
        faces.append(ids)
        keys.append(np.nonzero(m)[0] * 5 + s)
    if not faces or sum(f.shape[0] for f in faces) == 0:
        return verts, np.zeros((0, 3), dtype=np.int32)
    faces, keys = np.concatenate(faces), np.concatenate(keys)
    return verts, np.ascontiguousarray(faces[np.argsort(keys, kind="stable")].astype(np.int32))


def smooth_gaussian(vol, sigma=1.5):
    """PyMCubes' smooth_gaussian: float64, the -0.5 offset, scipy's defaults (mode 'reflect', truncate 4.0)."""
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.asarray(vol, dtype=np.float64) - 0.5, sigma)


def iso_level(vol):
    v = np.asarray(vol, dtype=np.float64)
    return v.mean() + v.std() * 0.25


def edges_of(faces):
    """Undirected edges of a triangle list -> (unique [E, 2], use counts [E])."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    e.sort(axis=1)
    return np.unique(e, axis=0, return_counts=True)


def signed_volume(verts, faces):
    a, b, c = (verts[faces[:, i]].astype(np.float64) for i in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def face_normals(verts, faces):
    a, b, c = (verts[faces[:, i]].astype(np.float64) for i in range(3))
    return np.cross(b - a, c - a)


# ----------------------------------------------------------------------------------------------- test volumes and OBJ parsing
def _grid(R):
    x = np.arange(R, dtype=np.float64)
    return np.meshgrid(x, x, x, indexing="ij")


def sphere(R, r):
    """R^3 lattice of r - |x - c| (positive inside), c the lattice centre."""
    X, Y, Z = _grid(R)
    c = (R - 1) / 2
    return (r - np.sqrt((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2)).astype(np.float32)


def torus(R, big, small):
    X, Y, Z = _grid(R)
    c = (R - 1) / 2
    q = np.sqrt((X - c) ** 2 + (Y - c) ** 2) - big
    return (small - np.sqrt(q ** 2 + (Z - c) ** 2)).astype(np.float32)


def parse_obj(path):
    """-> (vertices [V, 3] float32, faces [F, 3] int64, 0-based) of an OBJ file holding only `v` and `f` lines"""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            tag, *rest = line.split()
            assert tag in ("v", "f")
            (v if tag == "v" else f).append(rest)
    return np.array(v, dtype=np.float32).reshape(-1, 3), np.array(f, dtype=np.int64).reshape(-1, 3) - 1
