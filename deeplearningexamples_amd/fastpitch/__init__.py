"""FastPitch (SpeechSynthesis/FastPitch) on the gfx950 library: text-to-mel inference on packed utterances."""
