from woft_amd.homography import (IRLSq_Huber, IRLSq_L1, find_homography_cvransac, find_homography_IRLSq_QR,  # noqa: F401
                                 find_homography_nonhomogeneous_QR, find_homography_TRS, torch_proj_errors)
