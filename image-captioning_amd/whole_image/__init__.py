"""The whole-image captioner (the reference's `image captioning/` package): model, pipeline, preprocess, train, predict (the
reference's test.py).  Image vectors come from generate_roi_features.generate_features(device_features=True)."""
