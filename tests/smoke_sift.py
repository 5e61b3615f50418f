"""smoke(): one small SIFT extraction on the GPU against what VLFeat gave for the same image (tests/golden/sift_vlfeat.npz)."""
import numpy as np


def run():
    import sift_cases as SC
    from colmap_amd import feature_extraction as FE
    c = SC.fixture()["odd67"]
    with FE.SiftFeatureExtractor(FE.SiftExtractionOptions(**c["options"])) as ex:
        kp, desc = ex.extract(c["image"])
    lo, hi = c["skip"], c["skip"] + c["num_out"]
    assert np.array_equal(kp.view(np.uint32), c["keypoints"][lo:hi].view(np.uint32)), "SIFT keypoints differ from VLFeat's"
    assert np.array_equal(desc, c["descriptors"][lo:hi]), "SIFT descriptors differ from VLFeat's"
    print(f"smoke: SIFT extraction HIP == VLFeat (bit-exact) on 67x45, {len(kp)} features")
