"""QuartzNet (SpeechRecognition/QuartzNet) on the gfx950 library: speech-to-text inference on packed utterances."""
