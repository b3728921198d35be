"""WaveGlow (SpeechSynthesis/Tacotron2, `-m WaveGlow`) on the gfx950 library: the training step and mel-to-audio inference
(SURVEY.md 8 row f1)."""
