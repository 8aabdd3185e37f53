"""The synthetic frame sequences of the part-detector tests (tests/test_gpu_parts.py on the GPU, tests/test_part_logic_cpu.py on the
CPU): a face that moves a little from frame to frame, and no face on every sixth frame (i % 6 == 4)."""


def scene(W, H, n, seed, two_faces=False):
    from nubovca import synth
    frames = []
    s = int(H * 0.5)
    for i in range(n):
        faces = [] if i % 6 == 4 else [(W // 5 + 5 * i, H // 5, s)]
        if two_faces and faces:
            faces.append((W // 2 + 30, H // 3 + 3 * i, int(s * 0.7)))
        frames.append(synth.make_bgr(W, H, seed + i, "natural", faces))
    return frames
