"""The reference's configuration dataclasses (PyTorch/DrugDiscovery/MoFlow/moflow/config.py) restated without rdkit: the same
fields, defaults and JSON, bond codes as plain names instead of rdkit bond types."""
import json
from dataclasses import asdict, dataclass, field
from typing import Dict, List, Optional

DUMMY_CODE = 0
CODE_TO_BOND_NAME = {0: "DUMMY", 1: "SINGLE", 2: "DOUBLE", 3: "TRIPLE"}
ATOM_VALENCY = {6: 4, 7: 3, 8: 2, 9: 1, 15: 3, 16: 2, 17: 1, 35: 1, 53: 1}


@dataclass
class DatasetConfig:
    dataset_name: str
    atomic_num_list: List[int]
    max_num_atoms: int
    labels: List[str]
    smiles_col: str
    code_to_atomic: Dict[int, int] = field(init=False)
    atomic_to_code: Dict[int, int] = field(init=False)
    valid_idx_file: str = field(init=False)
    csv_file: str = field(init=False)
    dataset_file: str = field(init=False)

    def __post_init__(self):
        self.valid_idx_file = "valid_idx_%s.json" % self.dataset_name
        self.csv_file = "%s.csv" % self.dataset_name
        self.dataset_file = "%s_relgcn_kekulized_ggnp.npz" % self.dataset_name
        self.code_to_atomic = dict(enumerate(sorted([DUMMY_CODE] + list(self.atomic_num_list))))
        self.atomic_to_code = {v: k for k, v in self.code_to_atomic.items()}


@dataclass
class AtomFlowConfig:
    n_flow: int
    hidden_gnn: List[int]
    hidden_lin: List[int]
    n_block: int = 1
    mask_row_size_list: List[int] = field(default_factory=lambda: [1])
    mask_row_stride_list: List[int] = field(default_factory=lambda: [1])


@dataclass
class BondFlowConfig:
    hidden_ch: List[int]
    conv_lu: int
    n_squeeze: int
    n_block: int = 1
    n_flow: int = 10


@dataclass
class ModelConfig:
    atom_config: AtomFlowConfig
    bond_config: BondFlowConfig
    noise_scale: float = 0.6
    learn_dist: bool = True


_INIT_FALSE = ("code_to_atomic", "atomic_to_code", "valid_idx_file", "csv_file", "dataset_file")


@dataclass
class Config:
    dataset_config: DatasetConfig
    model_config: ModelConfig
    max_num_nodes: Optional[int] = None
    num_node_features: Optional[int] = None
    num_edge_features: int = len(CODE_TO_BOND_NAME)
    z_dim: int = field(init=False)

    def __post_init__(self):
        if self.max_num_nodes is None:
            self.max_num_nodes = self.dataset_config.max_num_atoms
        if self.num_node_features is None:
            self.num_node_features = len(self.dataset_config.code_to_atomic)
        self.z_dim = self.max_num_nodes ** 2 * self.num_edge_features + self.max_num_nodes * self.num_node_features

    def save(self, path):
        self.path = path
        with open(path, "w") as f:
            json.dump(asdict(self), f, indent=4, sort_keys=True)

    @classmethod
    def load(cls, path):
        """The JSON that save() writes (nested dictionaries, the derived fields included) -> Config."""
        with open(path) as f:
            d = json.load(f)
        ds = {k: v for k, v in d["dataset_config"].items() if k not in _INIT_FALSE}
        mc = d["model_config"]
        model = ModelConfig(AtomFlowConfig(**mc["atom_config"]), BondFlowConfig(**mc["bond_config"]),
                            **{k: v for k, v in mc.items() if k not in ("atom_config", "bond_config")})
        return cls(DatasetConfig(**ds), model, **{k: d[k] for k in ("max_num_nodes", "num_node_features", "num_edge_features") if k in d})

    def __repr__(self):
        return json.dumps(asdict(self), indent=4, separators=(",", ": "))


ZINC250K_CONFIG = Config(
    max_num_nodes=40,
    dataset_config=DatasetConfig(dataset_name="zinc250k", atomic_num_list=[6, 7, 8, 9, 15, 16, 17, 35, 53], max_num_atoms=38,
                                 labels=["logP", "qed", "SAS"], smiles_col="smiles"),
    model_config=ModelConfig(AtomFlowConfig(n_flow=38, hidden_gnn=[256], hidden_lin=[512, 64]),
                             BondFlowConfig(n_squeeze=20, hidden_ch=[512, 512], conv_lu=2)))

# the configuration of tests/golden/moflow_* (tools/make_moflow_fixture.py): every path of the generator at sizes a test can afford
FIXTURE_CONFIG = Config(
    max_num_nodes=8,
    dataset_config=DatasetConfig(dataset_name="fixture", atomic_num_list=[6, 7, 8], max_num_atoms=7, labels=["logP"], smiles_col="smiles"),
    model_config=ModelConfig(AtomFlowConfig(n_flow=10, hidden_gnn=[16], hidden_lin=[32, 8]),
                             BondFlowConfig(n_squeeze=4, hidden_ch=[32, 32], conv_lu=2, n_flow=3)))

CONFIGS = {"zinc250k": ZINC250K_CONFIG}
