"""Image front end with the reference's module names (data_processing/foerstner.py, point_features.py,
keypoint_extraction.py, fissure_enhancement.py): from a CT volume and a lung mask to the (C, K) point cloud the point networks consume;
and the way back from predicted lobe labels to fissures (random_walk.py, find_lobes.py)."""
