from woft_amd.homography import (IRLSq_Huber, IRLSq_L1, find_homography_cvransac, find_homography_IRLSq_QR,  # noqa: F401
                                 find_homography_nonhomogeneous_QR, find_homography_TRS, reproj_errors, torch_e2p,
                                 torch_H_proj, torch_p2e, torch_proj_diff_errors, torch_proj_errors, torch_reproj_errors)
