"""smoke(): the statistics of one small model (6 images, 150 points) on cuda:0 through colmap_amd.model_statistics,
checked against the sequential checker colmap_amd.workspace.Model (test infrastructure; imported only from
__graft_entry__.smoke()). Reads nothing outside the repository: the model is generated here."""
import numpy as np


def run():
    from colmap_amd import model_statistics as MS
    from colmap_amd import workspace as W
    rng = np.random.default_rng(3)
    m = W.Model()
    K = np.array([[100, 0, 50], [0, 100, 50], [0, 0, 1]], np.float32)
    for i in range(6):  # a row of cameras at z = -4 looking down +z; R = I and T on a grid: exact projection centres
        m.images.append(W.ModelImage("", 100, 100, K, np.eye(3, dtype=np.float32), np.array([-0.75 * i, 0, 4], np.float32)))
    for X in rng.uniform(-1, 1, (150, 3)).astype(np.float32):
        track = rng.choice(6, int(rng.integers(1, 6)), replace=False)
        m.points.append(W.ModelPoint(float(X[0]), float(X[1]), float(X[2]), [int(t) for t in track]))
    got, want = np.array(MS.compute_depth_ranges(m)), np.array(m.ComputeDepthRanges())
    assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), "depth ranges differ from the checker"
    assert MS.compute_shared_points(m) == m.ComputeSharedPoints(), "shared-point counts differ from the checker"
    got, want = MS.compute_triangulation_angles(m, 75.0), m.ComputeTriangulationAngles(75.0)
    for a, b in zip(got, want):
        assert sorted(a) == sorted(b) and all(abs(a[o] - b[o]) <= 4 * 2.0 ** -23 * b[o] for o in b), \
            "percentile triangulation angles differ from the checker"
    assert MS.get_max_overlapping_images(m, 3, 0.0) == m.GetMaxOverlappingImages(3, 0.0), "overlap lists differ"
    print("smoke: model statistics HIP == checker on 6 images, 150 points (depth ranges, shared points, angles, overlap)")
