"""Predictions -> molecules (reference: moflow/utils.py:47-158).  decode_predictions is postprocess_predictions on tensors; the rest
needs rdkit, which is imported on use: require_rdkit() says so in one line when it is missing."""
import re

import numpy as np
import torch

from .config import ATOM_VALENCY, DUMMY_CODE


def require_rdkit(what):
    try:
        from rdkit import Chem, RDLogger
    except ImportError:
        raise SystemExit("%s needs the rdkit package, which is not installed: write atomic numbers and bond codes with "
                         "--predictions_path X.npz instead" % what)
    RDLogger.DisableLog("rdApp.*")
    return Chem


def decode_predictions(code, x, config):
    """postprocess_predictions (utils.py:47-63): bond code [B, N, N] (the argmax over the bond types) and x [B, N, T], on any device ->
    (atomic numbers int64 [B, n], bond codes int64 [B, n, n]) as numpy with ONE host read, n = max_num_atoms."""
    n = config.dataset_config.max_num_atoms
    codes = config.dataset_config.code_to_atomic
    table = torch.tensor([codes[k] for k in range(len(codes))], dtype=torch.int64, device=x.device)
    atoms = table[torch.argmax(x[:, :n], dim=2)]
    both = torch.cat([atoms, code[:, :n, :n].reshape(code.shape[0], -1).to(torch.int64)], 1).cpu().numpy()
    return both[:, :n], both[:, n:].reshape(-1, n, n)


def _bond_types(Chem):
    return {1: Chem.rdchem.BondType.SINGLE, 2: Chem.rdchem.BondType.DOUBLE, 3: Chem.rdchem.BondType.TRIPLE}


def check_valency(Chem, mol):
    """(True, None), or (False, [atom index, valence]) read from rdkit's message."""
    try:
        Chem.SanitizeMol(mol, sanitizeOps=Chem.SanitizeFlags.SANITIZE_PROPERTIES)
        return True, None
    except ValueError as err:
        text = str(err)
        return False, [int(v) for v in re.findall(r"\d+", text[text.find("#"):])]


def construct_mol(Chem, atoms, bonds):
    """utils.py:74-101: the atoms that exist, the lower-triangle bonds, a +1 formal charge on N / O / S one bond over their valency."""
    kinds = _bond_types(Chem)
    exist = atoms != 0
    atoms, bonds = atoms[exist], bonds[exist][:, exist]
    mol = Chem.RWMol()
    for a in atoms:
        mol.AddAtom(Chem.Atom(int(a)))
    for start, end in zip(*np.where(bonds != DUMMY_CODE)):
        if start > end:
            mol.AddBond(int(start), int(end), kinds[int(bonds[start, end])])
            ok, where = check_valency(Chem, mol)
            if not ok:
                assert len(where) == 2
                idx, valence = where
                an = mol.GetAtomWithIdx(idx).GetAtomicNum()
                if an in (7, 8, 16) and valence - ATOM_VALENCY[an] == 1:
                    mol.GetAtomWithIdx(idx).SetFormalCharge(1)
    return mol


def correct_mol(Chem, mol):
    """utils.py:133-158: lower the highest-order bond of an over-valent atom until none is left; keep the largest fragment."""
    kinds = _bond_types(Chem)
    ok, where = check_valency(Chem, mol)
    while not ok:
        assert len(where) == 2
        queue = sorted(((b.GetIdx(), int(b.GetBondType()), b.GetBeginAtomIdx(), b.GetEndAtomIdx())
                        for b in mol.GetAtomWithIdx(where[0]).GetBonds()), key=lambda q: q[1], reverse=True)
        if queue:
            _, order, start, end = queue[0]
            mol.RemoveBond(start, end)
            if order - 1 >= 1:
                mol.AddBond(start, end, kinds[order - 1])
        ok, where = check_valency(Chem, mol)
    return max(Chem.GetMolFrags(mol, asMols=True), key=lambda m: m.GetNumAtoms())


def predictions_to_mols(Chem, atoms, bonds, correct_validity=False):
    mols = [construct_mol(Chem, a, b) for a, b in zip(atoms, bonds)]
    return [correct_mol(Chem, m) for m in mols] if correct_validity else mols
