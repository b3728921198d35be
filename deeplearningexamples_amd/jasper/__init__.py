"""Jasper (SpeechRecognition/Jasper) on the gfx950 library: speech-to-text inference on packed utterances."""
